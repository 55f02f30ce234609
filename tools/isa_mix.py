#!/usr/bin/env python3
"""Instruction mix per kernel instance from hipcc's ISA (--save-temps), compiled with the flags __graft_entry__.SOURCES gives the file.
    python tools/isa_mix.py gat_layer_fused.hip [substring ...]
Straight-line counts (the fused kernels are fully unrolled; loops are counted once)."""
import collections, importlib.util, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_isa(root, name, extra=()):
    """Compile csrc/<name> of the checkout at `root` with that checkout's own SOURCES flags (+ extra) and split the ISA per kernel:
    [(demangled name without 'void bgnn::' and the argument list, text up to the function-end label)].  tools/isa_diff.py shares it."""
    spec = importlib.util.spec_from_file_location("_ge_" + re.sub(r"\W", "_", root), os.path.join(root, "__graft_entry__.py"))
    ge = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ge)
    src = os.path.join(root, "bathymetric-gnn_amd", "csrc", name)
    with tempfile.TemporaryDirectory() as td:
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", "x.o", "-Wno-unused-result",
                        "--save-temps"] + list(ge.SOURCES.get(name, [])) + list(extra), cwd=td, check=True, capture_output=True)
        s = open(os.path.join(td, name.replace(".hip", "") + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    parts = re.split(r"\n(_Z\w+): +; @\w+\n", s)
    names, bodies = parts[1::2], parts[2::2]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = []
    for d, b in zip(dem, bodies):
        d = re.sub(r"\(.*", "", d).replace("void bgnn::", "")
        if "kernel" in d:
            out.append((d, b.split(".Lfunc_end")[0]))
    return out


def instructions(body):
    return [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]


if __name__ == "__main__":
    name, flt = sys.argv[1], sys.argv[2:]
    for d, body in kernel_isa(ROOT, name):
        if flt and not any(f in d for f in flt):
            continue
        c = collections.Counter()
        for l in instructions(body):
            i = l.split()[0]
            k = ("mfma" if i.startswith("v_mfma") else "trans" if re.match(r"v_(exp|rcp|log|sqrt|rsq|sin|cos)", i) else
                 "valu_pk" if i.startswith("v_pk_") else "valu_f64" if re.search(r"_f64", i) and i.startswith("v_") else "valu" if i.startswith("v_") else
                 "lds" if i.startswith("ds_") else "vmem" if i.startswith(("global_", "buffer_", "scratch_")) else "waitcnt" if i.startswith("s_waitcnt") else
                 "barrier" if i.startswith("s_barrier") else "salu" if i.startswith("s_") else "other")
            c[k] += 1
        print(f"{d[:60]:60s}", " ".join(f"{k} {v}" for k, v in sorted(c.items())))
