"""Record tests/golden/route_census.json: the ``_lib`` calls every case of tests/route_cases.py makes, and what comes back.

    python tools/record_route_census.py --tree CHECKOUT --commit HASH tests/golden/route_census.json

``CHECKOUT`` is a built checkout of the commit to record FROM - the commit before the typed route record, never the code under
test - whose ``selfpose3d_amd`` is put in front of the path (a ``git worktree`` of that commit, say); the cases and the
recording wrappers are this tree's tests/route_cases.py, which uses only names that commit has.  ``HASH`` goes into the file's
``recorded_from`` field.  Needs a GPU: the wrappers call through.  tests/test_gpu_route_census.py holds later trees to the file;
a case changed on purpose gets an entry ``{"outcome": ..., "reason": ...}`` in the file's ``intended`` block by hand; the
recorded outcome stays."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--commit", required=True)
    ap.add_argument("out")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    import selfpose3d_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(selfpose3d_amd.__file__))) == os.path.abspath(a.tree), selfpose3d_amd.__file__
    import importlib.util               # this tree's cases: CHECKOUT has a tests package of its own in front of the path
    spec = importlib.util.spec_from_file_location("route_cases", os.path.join(HERE, "tests", "route_cases.py"))
    route_cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(route_cases)
    all_cases = route_cases.all_cases
    dev = torch.device("cuda:0")
    table = {}
    for cid, runner, case in all_cases():
        table[cid] = json.loads(json.dumps(runner(case, dev)))
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    intended = {}
    if os.path.exists(a.out):           # entries written by hand survive a new recording
        with open(a.out) as fh:
            intended = json.load(fh).get("intended", {})
    groups = {}                         # many cases share an outcome: one line per distinct outcome, with its cases
    for cid, got in table.items():
        groups.setdefault(json.dumps(got, separators=(",", ":")), []).append(cid)
    with open(a.out, "w") as fh:
        fh.write('{"recorded_from": %s,\n "intended": {\n' % json.dumps(a.commit))
        fh.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in intended.items()))
        fh.write('\n },\n "outcomes": [\n')
        fh.write(",\n".join('  {"cases": %s, "outcome": %s}' % (json.dumps(ids), got) for got, ids in groups.items()))
        fh.write("\n ]\n}\n")
    raised = sum(1 for v in table.values() if isinstance(v, list))
    print("wrote", a.out, len(table), "cases,", raised, "of them refusals")


if __name__ == "__main__":
    main()
