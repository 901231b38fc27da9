#!/usr/bin/env python3
"""Record a family of tests/golden/walk_bits*.json: per case of tests/test_walk_bits_gpu.py the SHA-256 of the output bytes, the
kernels of the launch log and the workspace size, from the library CASYNC_LIB names -- a build of the PARENT of the commit under
test, never the in-tree library:

    git worktree add /tmp/parent <parent commit> && (cd /tmp/parent && python -m calipsync_amd.build)
    CASYNC_LIB=/tmp/parent/calipsync_amd/lib/libcasync_hip.so python tools/record_walk_bits.py --family sync --commit <parent commit>

--family names the handles recorded and thereby the file (the test's GOLDEN): `walk` is S3FD and HuBERT in walk_bits.json, `sync`
SyncNet_color in walk_bits_sync.json, `unet` the U-Net plan in walk_bits_unet.json.  Each file has its own parent commit;
recording one leaves the others as they are.

The case table and the run are the test's own (imported from it), so the two cannot drift apart.  Every case runs twice: a
recording with an output that is not finite, or with a case that does not repeat itself, is refused.

The `unet` family runs every case three times.  Kernels, profiled rows and workspace sizes have to repeat in every case, and so
have the hashes of every `sk0` case (gemm_streamk=0): otherwise nothing is written.  A `default` case whose hashes do not repeat
keeps the rest; its hashes are written as null beside the reason, and the count of such cases is printed."""
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
    ap.add_argument("--family", required=True, choices=("walk", "sync", "unet"), help="the handles to record: the file of that family is written")
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
    if args.family == "unet":
        return record_unet(T, args.commit, hipcc, out)
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


def record_unet(T, commit, hipcc, out):
    cases, refused, no_hashes = {}, [], []
    for name in (n for n in T.CASES if T.family(n) == "unet"):
        runs = [T.record(name) for _ in range(3)]
        rec = cases[name] = runs[0]
        hashed = ("out", "taps")
        if any({k: v for k, v in r.items() if k not in hashed} != {k: v for k, v in rec.items() if k not in hashed} for r in runs[1:]):
            refused.append(name + " (kernels, rows or workspace)")
        elif any(r != rec for r in runs[1:]):
            differ = sorted({"out" for r in runs[1:] if r["out"] != rec["out"]} | {t for r in runs[1:] for t in rec["taps"] if r["taps"][t] != rec["taps"][t]})
            if T.CASES[name][5] != "default":
                refused.append(f"{name} ({', '.join(differ)})")
            no_hashes.append(name)
            rec.update(out=None, taps={t: None for t in rec["taps"]}, unstable=f"differed between three runs of commit {commit[:12]}: {', '.join(differ)}")
        print(f"{name}: workspace {rec['workspace']}  {(rec.get('out') or '-')[:16]}  {len(rec.get('rows', []))} rows  {rec.get('unstable', '')}")
    if refused:
        sys.exit(f"cases that have to repeat themselves on this library and do not (nothing written): {refused}")
    write_unet(T, out, commit, hipcc, cases)
    print(f"wrote {out}: {len(cases)} cases, {len(no_hashes)} `default` cases without hashes: {no_hashes}")


def write_unet(T, out, commit, hipcc, cases):
    tables, packed = T.unet_pack(cases)
    with open(out, "w") as f:     # one table and one case per line
        f.write(json.dumps({"parent_commit": commit, "hipcc_version": hipcc}, indent=1)[:-2] + ",\n")
        f.write("".join(f' {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))},\n' for k, v in tables.items()))
        f.write(' "cases": {\n' + ",\n".join(f'  {json.dumps(n)}: {json.dumps(r, separators=(",", ":"))}' for n, r in packed.items()) + "\n }\n}\n")


if __name__ == "__main__":
    main()
