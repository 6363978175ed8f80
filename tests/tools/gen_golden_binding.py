"""Writes tests/golden/binding_calls.json: what every case of tests/binding_cases.py makes mdrp_amd/_capi.py hand to the library (recorded by a stub,
so neither a GPU nor the built library is needed), what it returns, the refusals the binding raises itself, and the signatures of every public
callable of mdrp_amd._capi and mdrp_amd.poselib, for tests/test_binding_calls_host.py.

    python tests/tools/gen_golden_binding.py [--check | --only SECTION] [OUT.json]

--check compares with the committed fixture instead of writing it; --only SECTION[,SECTION] (calls | refusals | missing | signatures) rewrites those
sections and keeps the rest of the committed file.  The committed file pins the binding as it was before its copies were folded; only its "missing" section (the
wording of the missing-symbol refusal) was regenerated afterwards.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import binding_cases as bc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "binding_calls.json")


def main(argv):
    doc = json.loads(json.dumps(bc.snapshot()))
    out = next((a for a in argv if a.endswith(".json")), OUT)
    if "--check" in argv:
        with open(out) as f:
            want = json.load(f)
        bad = [(s, k) for s in want for k in set(want[s]) | set(doc[s]) if want[s].get(k) != doc[s].get(k)]
        assert not bad, bad[:20]
        print(f"{sum(len(v) for v in doc.values())} entries match {out}")
        return
    if "--only" in argv:
        sections = argv[argv.index("--only") + 1].split(",")
        with open(out) as f:
            doc = {**json.load(f), **{s: doc[s] for s in sections}}
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['calls'])} cases, {len(doc['refusals'])} refusals, {len(doc['missing'])} missing symbols -> {out}")


if __name__ == "__main__":
    main(sys.argv[1:])
