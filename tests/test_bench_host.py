"""Host-side logic of bench.py that needs no GPU: how many CPUs / GPUs the process may really use."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_usable_cpus_respects_the_affinity_mask():
    b = _bench()
    usable, cpu_count, affinity, quota = b.usable_cpus()
    assert 1 <= usable <= affinity <= max(cpu_count, affinity)
    if quota is not None:
        assert usable <= max(1, int(quota + 0.999))
    # a child pinned to one CPU must report one usable CPU whatever os.cpu_count() says
    one = sorted(os.sched_getaffinity(0))[0]
    code = ("import os,sys,importlib.util; os.sched_setaffinity(0,{%d}); "
            "s=importlib.util.spec_from_file_location('b', %r); m=importlib.util.module_from_spec(s); s.loader.exec_module(m); "
            "print(m.usable_cpus()[0])" % (one, os.path.join(ROOT, "bench.py")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert r.stdout.strip() == "1"


def test_gpu_count_does_not_load_torch_and_honours_visible_devices(monkeypatch):
    code = ("import sys,importlib.util; "
            "s=importlib.util.spec_from_file_location('b', %r); m=importlib.util.module_from_spec(s); s.loader.exec_module(m); "
            "n=m.visible_gpu_count(); print(n, 'torch' in sys.modules)" % os.path.join(ROOT, "bench.py"))
    env = dict(os.environ)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True, env=env)
    n, torch_loaded = r.stdout.split()
    has_kfd = os.path.isdir("/sys/class/kfd/kfd/topology/nodes")
    assert int(n) >= 0
    if has_kfd:
        assert torch_loaded == "False"  # the launcher parent counts GPUs from sysfs alone
        env["HIP_VISIBLE_DEVICES"] = ""
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True, env=env)
        assert r.stdout.split()[0] == "0"


def test_dump_outputs_writes_float32_and_samples_above_the_cap(tmp_path, monkeypatch):
    import numpy as np

    from pcl_tracking_amd.scene import PARTICLE_DTYPE

    b = _bench()
    rng = np.random.default_rng(3)

    def outs(n_obj, n):
        o = []
        for _ in range(n_obj):
            p = rng.standard_normal((n, 8)).astype(np.float32).view(PARTICLE_DTYPE).reshape(-1)
            o.append((p[0].copy(), p))
        return o

    small = outs(2, 100)
    b.dump_outputs(str(tmp_path / "a"), small)
    res, part = np.load(tmp_path / "a" / "result.npy"), np.load(tmp_path / "a" / "particles.npy")
    assert res.dtype == np.float32 and res.shape == (2, 8) and part.dtype == np.float32 and part.shape == (2, 100, 8)
    assert np.array_equal(part[1], small[1][1].view(np.float32).reshape(-1, 8))
    assert np.array_equal(res[0], part[0, 0]) and not (tmp_path / "a" / "particles_index.npy").exists()

    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 4096)
    big = outs(2, 1000)
    for d in ("b", "c"):
        b.dump_outputs(str(tmp_path / d), big)
    total = sum(os.path.getsize(tmp_path / "b" / f) - 128 for f in os.listdir(tmp_path / "b"))  # less the .npy headers
    assert total <= 4096
    idx = np.load(tmp_path / "b" / "particles_index.npy")
    part = np.load(tmp_path / "b" / "particles.npy")
    assert idx.dtype == np.float64 and len(idx) > 0 and np.all(np.diff(idx) > 0) and part.shape == (2, len(idx), 8)
    assert np.array_equal(part[0], big[0][1].view(np.float32).reshape(-1, 8)[idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(tmp_path / "c" / "particles_index.npy"))  # the sample is fixed
