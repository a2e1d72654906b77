"""Every forward-unprojection request of tests/fwd_request_cases.py - six entries x three layout bytes x all 512 flag words x the
shape cases - against tests/golden/fwd_request_census.json, the answers of the library BEFORE the request became a typed record
(tools/record_fwd_request_census.py recorded them from the real entries of that commit, not from the code under test).

* the plan entry (sp3d_unproject_fwd_plan: no HIP call, runs everywhere) gives the recorded code, launches - kernel name and
  every PLAN_FIELDS value - and tuning for every request;
* where no GPU is visible, the real entries called with dummy pointers give the recorded refusal, or a positive code (HIP
  finds no device) where the request is accepted: the plan answers what the entry answers.  The pointer-fact cases (result
  misaligned, grids given) have no plan and are held here only.

The requests on which the previous plan entry and the previous real entries disagreed are listed in the file (`plan_disagreed`);
the recorded answer is the entry's."""
import json
import os

import pytest
import torch

from selfpose3d_amd import _lib, build as sbuild
from tests.fwd_request_cases import FLAG_WORDS, LAYOUT_BYTES, Asker, cases, flags_of, has_layout_word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ask():
    sbuild.build()
    return Asker(_lib.load())


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "golden", "fwd_request_census.json")) as fh:
        c = json.load(fh)
    c["outcomes"] = [(rc, tuple(tuple(l) for l in launches), None if tuning is None else tuple(tuning)) for rc, launches, tuning in c["outcomes"]]
    return c


def unroll(runs):
    out = [v for v, n in runs for _ in range(n)]
    assert len(out) in (1, FLAG_WORDS)
    return out


def test_the_census_covers_the_cases(census):
    want = {f"{c['entry']}/{layout}/{c['id']}" for c in cases() for layout in LAYOUT_BYTES}
    assert set(census["cases"]) == want and len(want) * FLAG_WORDS > 200000
    assert set(census["facts"]) == {f"{c['entry']}/{layout}/{c['id']}" for c in cases(facts=True) for layout in LAYOUT_BYTES}
    assert set(census["plan_disagreed"]) <= want
    # the six disagreements the typed request was written to end, among the listed ones: the strided and the training entry
    # refuse a degenerate image, a planar tensor without the one-channel flag, a channels-last result and bf16 storage
    listed = {(k, i) for k, runs in census["plan_disagreed"].items() for a, b in runs for i in range(a, b + 1)}
    for key, word in (("strided/1/img18x1_jp16", 0), ("strided/1/jp16_J16_z32", 1), ("strided/0/jp16_J15", 0), ("train/1/img18x1_jp16", 0),
                      ("train/0/jp16_J15", 0), ("train/1/jp16_J15", 2)):
        assert (key, word) in listed and census["outcomes"][unroll(census["cases"][key])[word]][0] == -4, (key, word)


def test_the_plan_answers_what_the_previous_entries_answered(ask, census):
    outcomes, wrong = census["outcomes"], []
    for c in cases():
        for layout in LAYOUT_BYTES:
            want = unroll(census["cases"][f"{c['entry']}/{layout}/{c['id']}"])
            for i in range(FLAG_WORDS):
                got = ask.ask_plan(c, layout, flags_of(i))
                if got != outcomes[want[i]]:
                    wrong.append((c["entry"], layout, c["id"], hex(flags_of(i)), got[0], outcomes[want[i]][0]))
    assert not wrong, (len(wrong), wrong[:20])


def test_the_entries_answer_what_the_plan_answers(ask, census):
    """dummy pointers that are never dereferenced: an accepted request reaches HIP, which finds no device - only where no GPU is
    visible (the GPU suites run the accepted requests with real tensors)"""
    if torch.cuda.is_available():
        pytest.skip("dummy-pointer refusals are checked only where no GPU is visible")
    outcomes, wrong = census["outcomes"], []
    for facts in (False, True):
        for c in cases(facts):
            for layout in LAYOUT_BYTES:
                runs = unroll(census["facts" if facts else "cases"][f"{c['entry']}/{layout}/{c['id']}"])
                for i in range(FLAG_WORDS if has_layout_word(c["entry"]) else 1):
                    want = runs[i] if facts else outcomes[runs[i]][0]
                    got = ask.ask_entry(c, layout, flags_of(i))
                    if (got != want) if want < 0 else (got <= 0):
                        wrong.append((c["entry"], layout, c["id"], hex(flags_of(i)), got, want))
    assert not wrong, (len(wrong), wrong[:20])
