#!/usr/bin/env python3
"""Records tests/golden/ref_run/*.json from a build of the reference's own units.

Run where oracle/_ref/libbrb_ref.so exists (oracle/ref_build/Makefile builds it from a checkout of the
reference; __graft_entry__.build() calls it).  Every family of tests/ref_run_cases.py is run against that
library and what it returns is written as one JSON file per family.  The files hold inputs, outputs and
hashes only.  Two runs write identical files.

    python tests/golden/make_ref_run.py            # write the files
    python tests/golden/make_ref_run.py --check    # compare with the committed files, write nothing
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import ref_run_cases as rr  # noqa: E402

MAX_BYTES = 61440          # no file larger than the largest of the other fixtures (digests.json)


def text_of(obj) -> str:
    """Compact JSON, keys of the outer level sorted, its dicts one entry per line -- short entries share a line."""
    def line(v):
        return json.dumps(v, sort_keys=True, separators=(",", ":"))
    out = ["{"]
    top = sorted(obj)
    for i, k in enumerate(top):
        v, end = obj[k], "" if i == len(top) - 1 else ","
        if isinstance(v, dict) and len(line(v)) > 160:
            out.append(f" {json.dumps(k)}:{{")
            lines = []
            for j in v:                                      # the order the family produced: its cases' order
                e = f"{json.dumps(j)}:{line(v[j])}"
                if lines and len(lines[-1]) + len(e) < 160:
                    lines[-1] += "," + e
                else:
                    lines.append("  " + e)
            out += [x + "," for x in lines[:-1]] + lines[-1:]
            out.append(" }" + end)
        else:
            out.append(f" {json.dumps(k)}:{line(v)}{end}")
    out.append("}")
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of writing them")
    args = ap.parse_args()
    if not os.path.exists(rr.REF_LIB):
        print(f"{rr.REF_LIB} is missing: build it with `make -C oracle/ref_build`", file=sys.stderr)
        return 2
    api = rr.RefApi()
    os.makedirs(rr.REF_DIR, exist_ok=True)
    bad = 0
    for fam in rr.FAMILIES:
        text = text_of(rr.FAMILY_FN[fam](api))
        path = os.path.join(rr.REF_DIR, fam + ".json")
        assert len(text) <= MAX_BYTES, f"{fam}.json would be {len(text)} bytes"
        if args.check:
            same = os.path.exists(path) and open(path).read() == text
            print(f"{fam}.json: {'same' if same else 'DIFFERS'} ({len(text)} bytes)")
            bad += not same
        else:
            with open(path, "w") as f:
                f.write(text)
            print(f"{fam}.json: {len(text)} bytes")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
