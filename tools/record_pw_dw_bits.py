#!/usr/bin/env python3
"""Record tests/golden/pw_dw_bits.json: per case of tests/test_pw_dw_bits_gpu.py the SHA-256 of the output bytes and the kernel
that ran, from the library CASYNC_LIB names -- a build of the PARENT of the commit under test, never the in-tree library:

    git worktree add /tmp/parent <parent commit> && (cd /tmp/parent && python -m calipsync_amd.build)
    CASYNC_LIB=/tmp/parent/calipsync_amd/lib/libcasync_hip.so python tools/record_pw_dw_bits.py --commit <parent commit>

The case table and the launch are the test's own (imported from it), so the two cannot drift apart.  Every case must also meet
the test's float64 bound here: a recording from a broken library is refused."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="id of the commit CASYNC_LIB was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pw_dw_bits.json"))
    args = ap.parse_args()
    if not os.environ.get("CASYNC_LIB"):
        sys.exit("CASYNC_LIB must name a library built from the parent commit (the in-tree library is the code under test)")
    import torch
    from calipsync_amd import _lib
    import test_pw_dw_bits_gpu as T

    lib = _lib.load()
    try:
        hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()[0].strip()
    except (OSError, IndexError):
        hipcc = "unknown"
    cases = {}
    for name, case in T.CASES.items():
        got, ref, names = T.run_case(lib, name)
        err = T.rel_err(got, ref)
        assert not torch.isnan(got).any() and err < T.BOUND, (name, err)
        assert names == {case[8]}, (name, names)
        cases[name] = {"sha256": T.digest(got), "kernel": case[8]}
        print(f"{name}: {cases[name]['kernel']}  rel err {err:.3g}  {cases[name]['sha256'][:16]}")
    with open(args.out, "w") as f:
        json.dump({"parent_commit": args.commit, "hipcc_version": hipcc, "cases": cases}, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
