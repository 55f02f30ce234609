#!/usr/bin/env python3
"""Same instruction stream?  Compiles the named translation units of THIS tree and of another checkout of the repository (a `git worktree`
of the parent commit, say), each with its own __graft_entry__.SOURCES flags, and compares every kernel's ISA text, matched by demangled
name across the files (a kernel may have moved to another file):
    python tools/isa_diff.py [--diag] <other-tree> file.hip [file.hip ...]
A file one of the trees does not have is skipped there.  Before comparing, comments, the function-end labels and the
__hip_cuid_* symbol are dropped and the function number in block labels (.LBB<n>_<i>: it follows the kernel's place in its file) is
blanked; beyond that it is a plain text comparison.  --diag adds -DBGNN_DIAG=1.  Exit status 1 if anything differs, is new or is missing."""
import concurrent.futures, os, re, sys
from isa_mix import ROOT, instructions, kernel_isa


def normalised(body):
    keep = []
    for l in body.split("\n"):
        t = l.strip()
        if not t or t.startswith(";") or "__hip_cuid_" in t or t.startswith(".Lfunc_end"):
            continue
        keep.append(re.sub(r"\.LBB\d+_", ".LBB_", t.split(";")[0].rstrip()))     # (trailing comments name IR blocks by serial number)
    return keep


def tree_kernels(root, files, extra):
    files = [f for f in files if os.path.exists(os.path.join(root, "bathymetric-gnn_amd", "csrc", f))]
    if not files:
        return {}
    with concurrent.futures.ThreadPoolExecutor(len(files)) as ex:
        per_file = list(ex.map(lambda f: kernel_isa(root, f, extra), files))
    return {d: (f, body) for f, ks in zip(files, per_file) for d, body in ks}


def main(argv):
    extra = ["-DBGNN_DIAG=1"] if "--diag" in argv else []
    argv = [a for a in argv if a != "--diag"]
    if len(argv) < 2:
        sys.exit(__doc__)
    other, files = os.path.abspath(argv[0]), argv[1:]
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        fa, fb = ex.submit(tree_kernels, other, files, extra), ex.submit(tree_kernels, ROOT, files, extra)
        a, b = fa.result(), fb.result()
    bad = 0
    for d in sorted(set(a) | set(b)):
        if d not in a or d not in b:
            print(f"{'new' if d not in a else 'missing':9s} {d}")
            bad += 1
            continue
        same = normalised(a[d][1]) == normalised(b[d][1])
        bad += not same
        print(f"{'identical' if same else 'differs':9s} {d}  [{len(instructions(a[d][1]))} -> {len(instructions(b[d][1]))} instructions; {a[d][0]} -> {b[d][0]}]")
    print(f"{len(a)} kernels there, {len(b)} here, {bad} not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
