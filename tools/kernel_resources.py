#!/usr/bin/env python3
"""Register / scratch / LDS / occupancy table of every kernel in a .hip file, from hipcc's -Rpass-analysis=kernel-resource-usage
remarks, compiled with the flags __graft_entry__.SOURCES gives that file.  No GPU needed.
    python tools/kernel_resources.py gat_layer_fused.hip [substring ...]"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge

def dynamic_lds(dem):
    """gat_layer_fused_kernel<HC, 64, K, NT, EPI, 0, 0, LF> requests its LDS at launch (the remarks above say 0): ask the built library
    (bgnn_internal_fused_lds_bytes, a constexpr table over the same FusedLds the launcher uses).  None: not such a kernel / no library."""
    m = re.match(r"gat_layer_fused_kernel<(\d+), 64, (\d+), (\d+), (\d+), 0, 0, (\d+)>", dem)
    if not m or not os.path.exists(ge.LIB):
        return None
    import ctypes
    try:
        fn = ctypes.CDLL(ge.LIB).bgnn_internal_fused_lds_bytes
    except (OSError, AttributeError):
        return None
    hc, k, nt, epi, lf = (int(x) for x in m.groups())
    n = fn(hc, k, nt, epi, lf)
    return n if n >= 0 else None


def main():
    name = sys.argv[1]
    flt = sys.argv[2:]
    src = os.path.join(ROOT, "bathymetric-gnn_amd", "csrc", name)
    extra = list(ge.SOURCES.get(name, []))
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", "/dev/null", "-Wno-unused-result",
           "-Rpass-analysis=kernel-resource-usage"] + extra
    t = subprocess.run(cmd, capture_output=True, text=True).stderr
    blocks = re.split(r"remark: [^\n]*Function Name: ", t)[1:]
    filt = subprocess.run(["c++filt"], input="\n".join(b.split()[0] for b in blocks), capture_output=True, text=True).stdout.split("\n")
    for b, dem in zip(blocks, filt):
        g = lambda k: (re.search(k + r": (\d+)", b) or [None, "?"])[1]
        dem = dem.replace("bgnn::", "").replace("(anonymous namespace)::", "").replace("void ", "")
        dem = re.sub(r"\(.*", "", dem)
        if flt and not any(f in dem for f in flt):
            continue
        lds = g('LDS Size .bytes/block.')
        if lds == "0" and dynamic_lds(dem) is not None:
            lds = str(dynamic_lds(dem))
        print(f"{dem[:100]:100s} VGPR {g('VGPRs'):>3} AGPR {g('AGPRs'):>3} scratch {g('ScratchSize .bytes/lane.'):>4} occ {g('Occupancy .waves/SIMD.'):>2} LDS {lds:>6}")

main()
