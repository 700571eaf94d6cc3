"""Engine.step sends the device exactly what it sent when tests/golden/step_trace.json.gz was recorded: the same entry points with
the same arguments in the same order, the same waits on the sync's buckets and the same read-backs, in every mode of the step
without a sync, with collectives in flight and with collectives that have landed, on an engine built with share=, and across a
step the fp16 guard skips (tests/step_trace_ref.py has the scenarios and the normalisation; tools/step_trace.py records)."""
import os

import pytest

pytestmark = pytest.mark.gpu

import step_trace_ref as S                              # noqa: E402

_WANT = {}


def want(golden_dir):
    if not _WANT:
        _WANT.update(S.load(os.path.join(golden_dir, "step_trace.json.gz")))
    return _WANT


def test_fixture_holds_the_scenarios_of_the_list(golden_dir):
    assert sorted(want(golden_dir)) == sorted(S.scenarios())


@pytest.mark.parametrize("name", S.scenarios())
def test_step_trace_is_the_recorded_one(golden_dir, name):
    exp, got = want(golden_dir)[name], S.run(name)
    for i, (e, g) in enumerate(zip(exp, got)):
        if e != g:
            print("[step-trace] %s: entry %d differs\n  expected %s\n  got      %s" % (name, i, e, g))
            break
    else:
        if len(exp) != len(got):
            longer = exp if len(exp) > len(got) else got
            print("[step-trace] %s: %d entries expected, %d got; the first one beyond: %s" % (name, len(exp), len(got), longer[min(len(exp), len(got))]))
    assert got == exp, name
