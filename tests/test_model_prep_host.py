"""Host-side checks of the model preparation: no device means a loud failure, the Python wrappers refuse a wrong cloud
before they reach the library, and the flag parser create_model_amd now shares with auto_tracking_amd --segment
(examples/segment_options.hpp) left create_model_amd's usage text as it was."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pcl_tracking_amd import scene
from pcl_tracking_amd._lib import PftError

# create_model_amd's usage line before the parser moved into the shared header
OLD_USAGE = ("usage: %s <scene> --out DIR [--no-plane] [--transform 16 floats] "
             "[--box xmin,xmax,ymin,ymax,zmin,zmax] [--tolerance T] [--min-size N] [--max-size N] [--ascii] "
             "[--planes MAX[,FRACTION]] [--tree-refit] [--sac ITER,THRESHOLD] [--voxel LEAF]\n")


def test_no_gpu_means_loud_failure():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pcl_tracking_amd import _lib, model

    L = _lib.load()
    h = C.c_void_p()
    assert L.pft_model_create(0, C.byref(h)) == 4 and not h.value  # PFT_ERR_NO_DEVICE
    with pytest.raises(PftError) as e:
        model.ModelPreparation().prepare(scene.make_model(64))
    assert e.value.status == 4


def test_wrappers_refuse_a_wrong_cloud_before_the_library():
    from pcl_tracking_amd import model

    mp = model.ModelPreparation()
    good = scene.make_model(64)
    for bad in (np.zeros((8, 8), np.float32), np.zeros(8, np.float64), good.reshape(8, 8), good.tolist(),
                good.view(np.uint8)):
        with pytest.raises(PftError) as e:
            mp.prepare(bad)
        assert e.value.status == 1
        assert mp._h is None  # the library was not asked for a handle
    with pytest.raises(PftError) as e:
        mp.prepareDevice(0, -1)
    assert e.value.status == 1 and mp._h is None
    with pytest.raises(PftError):
        mp.counts()


def test_shared_flag_parser_keeps_create_model_amds_usage_text():
    from pcl_tracking_amd import build

    exe = build.build_create_model_example()
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2
    assert r.stderr == OLD_USAGE % exe
    # a bad value of a shared flag is still refused by the flag's own message, in both drivers
    for exe, head in ((exe, ["scene", "--out", "d"]), (build.build_example(), ["--segment", "scene", "--frames", "f"])):
        r = subprocess.run([exe] + head + ["--planes", "99"], capture_output=True, text=True)
        assert r.returncode == 2 and r.stderr.startswith("--planes MAX[,FRACTION]")
    assert os.path.exists(os.path.join(os.path.dirname(build.EXAMPLES_DIR), "examples", "segment_options.hpp"))
