"""Every case of tests/route_cases.py makes the ``_lib`` calls, and returns the tensors or raises the error, that
tests/golden/route_census.json holds for it.  The file was recorded from the commit it names in ``recorded_from`` - the one
before the typed route record (``project_layer.Route``) - by tools/record_route_census.py, so it is what the scattered
predicates did, not what the record says.  A case changed on purpose has an entry in the file's ``intended`` block: the new
outcome and one sentence of reason; each is a place where two of the old predicates disagreed."""
import json
import os

import pytest
import torch

from tests import route_cases as rc

pytestmark = pytest.mark.gpu

MAX_INTENDED = 5


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(rc.ROOT, "tests", "golden", "route_census.json")) as fh:
        census = json.load(fh)
    census["cases"] = {cid: group["outcome"] for group in census["outcomes"] for cid in group["cases"]}     # one line per outcome
    return census


def _replay(census, cases, runner, ident):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda:0")
    wrong = []
    for c in cases:
        cid = ident(c)
        want = census["intended"][cid]["outcome"] if cid in census["intended"] else census["cases"][cid]
        got = json.loads(json.dumps(runner(c, dev)))
        if got != want:
            wrong.append((cid, want, got))
    assert not wrong, "%d of %d cases differ; the first:\n%s\nrecorded: %s\nnow:      %s" % ((len(wrong), len(cases)) + wrong[0])


def test_file_names_its_commit_and_its_cases(census):
    assert len(census["recorded_from"]) == 40 and int(census["recorded_from"], 16) >= 0
    assert sorted(census["cases"]) == sorted(cid for cid, _, _ in rc.all_cases())
    assert sum(len(group["cases"]) for group in census["outcomes"]) == len(census["cases"])
    assert len(census["intended"]) <= MAX_INTENDED and set(census["intended"]) <= set(census["cases"])
    for cid, entry in census["intended"].items():
        assert entry["outcome"] != census["cases"][cid] and len(entry["reason"]) > 20, cid


def test_layer_cases(census):
    _replay(census, rc.layer_cases(), rc.run_layer_case, rc.case_id)


def test_net_cases(census):
    _replay(census, rc.net_cases(), rc.run_net_case, rc.net_case_id)
