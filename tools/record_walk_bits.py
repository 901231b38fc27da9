#!/usr/bin/env python3
"""Record a family of tests/golden/walk_bits*.json: per case of tests/test_walk_bits_gpu.py the SHA-256 of the output bytes, the
kernels of the launch log and the workspace size, from the library CASYNC_LIB names -- a build of the PARENT of the commit under
test, never the in-tree library:

    git worktree add /tmp/parent <parent commit> && (cd /tmp/parent && python -m calipsync_amd.build)
    CASYNC_LIB=/tmp/parent/calipsync_amd/lib/libcasync_hip.so python tools/record_walk_bits.py --family sync --commit <parent commit>

--family names the handles recorded and thereby the file (the test's GOLDEN): `walk` is S3FD and HuBERT in walk_bits.json, `sync`
SyncNet_color in walk_bits_sync.json.  Each file has its own parent commit; recording one leaves the other as it is.

The case table and the run are the test's own (imported from it), so the two cannot drift apart.  Every case runs twice: a
recording with an output that is not finite, or with a case that does not repeat itself, is refused."""
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
    ap.add_argument("--family", required=True, choices=("walk", "sync"), help="the handles to record: the file of that family is written")
    ap.add_argument("--out", help="another place for the file")
    args = ap.parse_args()
    if not os.environ.get("CASYNC_LIB"):
        sys.exit("CASYNC_LIB must name a library built from the parent commit (the in-tree library is the code under test)")
    import test_walk_bits_gpu as T

    try:
        hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()[0].strip()
    except (OSError, IndexError):
        hipcc = "unknown"
    cases, unstable = {}, []
    out = args.out or T.GOLDEN[args.family]
    for name in (n for n in T.CASES if T.family(n) == args.family):
        cases[name] = T.record(name)
        if T.record(name) != cases[name]:
            unstable.append(name)
        print(f"{name}: workspace {cases[name]['workspace']}  {cases[name].get('sha256', '-')[:16]}  {cases[name].get('kernels', '')}")
    if unstable:
        sys.exit(f"cases that do not repeat themselves on this library (nothing written): {unstable}")
    with open(out, "w") as f:
        json.dump({"parent_commit": args.commit, "hipcc_version": hipcc, "cases": cases}, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
