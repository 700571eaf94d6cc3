"""CPU: tests/inbatch_steps_ref.py - the schedules tests/test_inbatch_steps_gpu.py drives a long-lived engine through with in-batch
negatives on and off - holds every step pair it is there for.  The pairs are read back from the records, so a schedule that was
thinned, or a record whose switch was flipped, fails here and not silently on the GPU."""
import pytest

import inbatch_ref as R
import inbatch_steps_ref as SR


@pytest.mark.parametrize("name", sorted(SR.SCHEDULES))
def test_every_required_pair_is_in_the_records(name):
    dtype = "fp16"
    recs = [r for r in SR.SCHEDULES[name] if r["only"] in (None, dtype)]
    seen = SR.pairs(recs)
    assert SR.REQUIRED[name] <= seen, sorted(SR.REQUIRED[name] - seen)
    if name != "scale":                                    # bf16 sees the same schedule
        assert [r for r in SR.SCHEDULES[name] if r["only"] in (None, "bf16")] == recs
    else:
        assert not [r for r in SR.SCHEDULES[name] if r["only"] in (None, "bf16")]


def test_the_schedules_together():
    assert set(SR.SCHEDULES) == set(SR.REQUIRED)
    allrecs = [r for s in SR.SCHEDULES.values() for r in s]
    assert any(r["on"] and not r["backward"] for r in allrecs) and any(not r["on"] and not r["backward"] for r in allrecs)
    assert {r["mid"] for r in allrecs if r["mid"]} == set(SR.PATHS)
    assert all(r["on"] for r in allrecs if r["mid"] or r["plan"] or r["drop"] or r["form"] == "tok")
    assert {r["mult"] for r in allrecs} == {0.5, 1.0, 2.0} and all(r["only"] == "fp16" for r in allrecs if r["mult"] != 1.0)
    for s in SR.SCHEDULES.values():                        # windows are whole, and each mixes the switch
        for win in SR.windows(s, "fp16"):
            assert len(win) == 1 or {r["on"] for r in win} == {True, False}
    # a pair that is not there is not reported
    assert "on -> off -> on" not in SR.pairs(SR.SCHEDULES["toggle"][1:]) | SR.pairs(SR.SCHEDULES["toggle"][:2])
    assert "window on, off" not in SR.pairs([r for r in SR.SCHEDULES["moving"] if not (r["micro"] and not r["on"])][:5])


def test_the_feeds_differ_and_collide():
    """e5 and e5b are unlike batches (a step that reads the other's buffers differs), e3 is no prefix of either; each meets the
    fixture condition (tests/test_inbatch_ref_cpu.py) - here: the counts the GPU test reads back are not all alike."""
    e5, e5b, e3 = (R.engine_feed(n) for n in ("e5", "e5b", "e3"))
    assert not (e5[1] == e5b[1]).all() and not (e5[0] == e5b[0]).all() and e3[1].shape == (3, 5)
    for f in (e5, e5b, e3):
        n = R.eligibility(f[0], f[1]).sum(1)
        assert n.min() == 0 and n.max() >= 2 and (R.eligibility_v(f[0], f[1]) == R.eligibility(f[0], f[1])).all()
