"""Writes tests/golden/entry_refusals.json: (return code, mdrp_last_error()) of every probe of tests/refusal_cases.py, for
tests/test_gpu_refusals.py.  Needs a GPU (a handle), and the library whose refusals are to be pinned: the one of the tree, or the one MDRP_LIB names
(the committed fixture was recorded from the library of the commit before the entry layer was single-sourced).

    python tests/tools/gen_golden_refusals.py [--check] [OUT.json]      (--check: compare with the committed fixture instead of writing it)

The file: {"messages": [...], "table": {entry point: {"defect" | "defect+defect": [return code, index into messages]}}}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refusal_cases as rc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "entry_refusals.json")


def pack(table):
    messages = sorted({m for probes in table.values() for _, m in probes.values()})
    index = {m: i for i, m in enumerate(messages)}
    return {"messages": messages, "table": {e: {d: [code, index[m]] for d, (code, m) in probes.items()} for e, probes in table.items()}}


def unpack(doc):
    return {e: {d: [code, doc["messages"][i]] for d, (code, i) in probes.items()} for e, probes in doc["table"].items()}


def main(argv):
    from mdrp_amd import _capi as capi
    h = capi.Handle(0)
    try:
        table = rc.run_table(capi.load_library(), rc.Base(capi, h._h))
    finally:
        h.close()
    accepted = [(e, d) for e, probes in table.items() for d, (code, _) in probes.items() if code == 0]
    assert not accepted, f"probes that were not refused: {accepted}"
    n = sum(len(p) for p in table.values())
    if "--check" in argv:
        with open(OUT) as f:
            want = unpack(json.load(f))
        bad = [(e, d, table[e].get(d), w) for e, probes in want.items() for d, w in probes.items() if table.get(e, {}).get(d) != w]
        assert not bad and n == sum(len(p) for p in want.values()), bad[:20]
        print(f"{n} probes match {OUT}")
        return
    out = next((a for a in argv if a.endswith(".json")), OUT)
    with open(out, "w") as f:
        json.dump(pack(table), f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{n} probes of {len(table)} entry points -> {out} ({capi.LIB_PATH})")


if __name__ == "__main__":
    main(sys.argv[1:])
