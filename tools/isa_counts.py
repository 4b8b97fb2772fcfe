"""Per-kernel instruction counts from the assembly of a device-only compile (hipcc ... --cuda-device-only -S):
    python tools/isa_counts.py FILE.s [SUBSTRING ...]
prints, for each kernel whose demangled name contains one of the substrings (all kernels without any), the number of
instructions in all, of ds_bpermute_b32, DPP, v_readlane_b32, s_barrier and s_waitcnt lgkmcnt(0) instructions and the VGPR / SGPR / scratch
figures of its .amdhsa block (profiles/small_kernel_tail.txt was made with it)."""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return names


def main():
    path, wanted = sys.argv[1], sys.argv[2:]
    text = open(path).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    pretty = dict(zip(kernels, demangle(kernels)))
    print("%-64s %6s %9s %5s %9s %9s %8s %5s %5s %7s" % ("kernel", "insts", "bpermute", "dpp", "readlane", "s_barrier", "lgkm(0)",
                                                          "vgpr", "sgpr", "scratch"))
    for k in kernels:
        name = re.sub(r"^void ", "", pretty[k]).split("(")[0]
        if wanted and not any(w in name for w in wanted):
            continue
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(k), text, re.M | re.S)
        body = m.group(1) if m else ""
        h = re.search(r"\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(k), text, re.S).group(1)

        def field(f):
            r = re.search(r"\.amdhsa_%s\s+(\d+)" % f, h)
            return r.group(1) if r else "?"
        # every instruction of the body: an indented mnemonic (labels, directives and comments are not)
        print("%-64s %6d %9d %5d %9d %9d %8d %5s %5s %7s" % (
            name[:64], len(re.findall(r"^\s+[a-z][a-z0-9_]+(?:\s|$)", body, re.M)),
            len(re.findall(r"\bds_bpermute_b32\b", body)), len(re.findall(r"_dpp\b", body)),
            len(re.findall(r"\bv_readlane_b32\b", body)), len(re.findall(r"\bs_barrier\b", body)),
            len(re.findall(r"s_waitcnt lgkmcnt\(0\)\s*$", body, re.M)), field("next_free_vgpr"), field("next_free_sgpr"),
            field("private_segment_fixed_size")))


if __name__ == "__main__":
    main()
