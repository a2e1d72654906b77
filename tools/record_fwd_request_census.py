"""Record tests/golden/fwd_request_census.json: what a library answers to every request of tests/fwd_request_cases.py.

    SP3D_LIB_PATH=<libsp3d.so of the commit to record> python tools/record_fwd_request_census.py tests/golden/fwd_request_census.json

The table is a record of the library it was run against (the parent of the commit that introduced the typed request), and
tests/test_fwd_request_census.py holds later libraries to it.  Per request:

  * the real extern "C" entry is called with dummy non-NULL pointers.  A negative code is the refusal; a positive one means the
    request was accepted and reached HIP, which finds no device.  That is only safe without a GPU, so the recorder refuses to
    run where one is visible.  (sp3d_unproject_fwd_zdft and _fwd_variant take no hm_layout: they are asked once per case, and
    their answer stands for flag word 0.)
  * the plan entry gives the launches and the tuning.
  * where the two disagree on accept / refuse, the ENTRY's answer is recorded and the request is listed under `plan_disagreed`
    (an accepted request the plan refuses would have no launches to record: the recorder stops there).

Format: `outcomes` holds each distinct answer once - [rc, launches, tuning], a launch being [name, PLAN_FIELDS...], launches and
tuning only for rc == 0.  `cases` maps "entry/layout byte/case id" to a run-length list [[outcome, count], ...] over the 512
flag words (word i = i << 8).  `facts` does the same for the pointer-fact cases, which only the real entries can be asked: its
runs hold the entry's code, 0 standing for "accepted".  `plan_disagreed` maps the same keys to [first, last] runs of flag words."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests.fwd_request_cases import FLAG_WORDS, LAYOUT_BYTES, Asker, cases, flags_of, has_layout_word  # noqa: E402


def rle(seq):
    runs = []
    for v in seq:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    return runs


def record(out):
    import torch
    from selfpose3d_amd import _lib
    if torch.cuda.is_available():
        sys.exit("a GPU is visible: the dummy-pointer calls of the accepted requests would launch on it")
    ask = Asker(_lib.load())
    ids, table, facts, disagreed = {}, {}, {}, {}
    for c in cases():
        once = None if has_layout_word(c["entry"]) else ask.ask_entry(c, 1, 0)
        for layout in LAYOUT_BYTES:
            row, bad = [], []
            for i in range(FLAG_WORDS):
                answer = ask.ask_plan(c, layout, flags_of(i))
                if once is None or i == 0:
                    rc = ask.ask_entry(c, layout, flags_of(i)) if once is None else once
                    if (rc < 0) != (answer[0] < 0) or (rc < 0 and rc != answer[0]):
                        assert rc < 0, ("accepted by the entry, refused by the plan", c, layout, i, rc, answer[0])
                        bad.append(i)
                        answer = (rc, (), None)
                row.append(ids.setdefault(answer, len(ids)))
            key = f"{c['entry']}/{layout}/{c['id']}"
            table[key] = rle(row)
            if bad:
                disagreed[key] = [[r[0], r[-1]] for r in _runs(bad)]
    for c in cases(facts=True):
        for layout in LAYOUT_BYTES:
            words = range(FLAG_WORDS) if has_layout_word(c["entry"]) else (0,)
            facts[f"{c['entry']}/{layout}/{c['id']}"] = rle(min(ask.ask_entry(c, layout, flags_of(i)), 0) for i in words)
    outcomes = [None] * len(ids)
    for answer, k in ids.items():
        outcomes[k] = [answer[0], [list(l) for l in answer[1]], list(answer[2]) if answer[2] is not None else None]
    with open(out, "w") as fh:
        fh.write('{\n "recorded_from": "194bc25",\n "outcomes": [\n' + ",\n".join("  " + json.dumps(o, separators=(",", ":")) for o in outcomes))
        for name, d in (("cases", table), ("facts", facts), ("plan_disagreed", disagreed)):
            fh.write(f'\n ],\n "{name}": {{\n' if name == "cases" else f'\n }},\n "{name}": {{\n')
            fh.write(",\n".join(f'  "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in d.items()))
        fh.write("\n }\n}\n")
    print("wrote", out, len(outcomes), "outcomes,", len(table), "plan rows,", len(facts), "fact rows,", len(disagreed), "rows with disagreements")


def _runs(idx):
    out = []
    for i in idx:
        if out and out[-1][-1] == i - 1:
            out[-1].append(i)
        else:
            out.append([i])
    return out


if __name__ == "__main__":
    record(sys.argv[1])
