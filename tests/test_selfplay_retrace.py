"""CPU: the checks of tests/selfplay_retrace.py on made-up records, so that the tail the composition tests share cannot pass when it
should not: assert_streams takes the right set and refuses each way of being wrong; the z back-fill; the Run is a cache key."""
import numpy as np
import pytest

import selfplay_retrace as SR


def _case():
    """three games of 3, 2 and 4 rows, the second game's first row written twice and its second left out; the device flushed them in
    the order 2, 0, 1"""
    rng = np.random.default_rng(1)
    games = [rng.integers(0, 256, (n, 265)).astype(np.uint8) for n in (3, 2, 4)]
    streams = [(games[0], None), (games[1], np.array([2, 0])), (games[2], np.ones(4, int))]
    records = np.concatenate([games[2], games[0], games[1][[0, 0]]])
    counters = dict(samples=9, decisions=31, simulations=200)
    return records, counters, streams, dict(decisions=31, simulations=200, samples=9)


def test_assert_streams_takes_the_right_set():
    SR.assert_streams(*_case())
    records, counters, streams, totals = _case()
    streams[1] = (streams[1][0], np.array([0, 0]))      # a game whose every record is left out: nothing of it to find
    SR.assert_streams(records[:7], dict(counters, samples=7), streams, totals)


def _flip(case):
    case[2][0][0][1, 100] ^= 1


def _apart(case):
    case[0][:] = case[0][[0, 1, 4, 2, 3, 5, 6, 7, 8]]   # game 2's last row behind game 0's first


def _missing(case):
    case[0][4:7] = case[0][0:3]                         # game 0's rows overwritten: the total still fits


def _one_more(case):
    case[0] = np.concatenate([case[0], case[0][-1:]])
    case[1]["samples"] = 10


def _samples(case):
    case[1]["samples"] = 8


def _decisions(case):
    case[3]["decisions"] = 30


def _simulations(case):
    case[1]["simulations"] = 202


def _empty(case):
    case[2][0] = (np.zeros((0, 265), np.uint8), None)
    case[0] = np.concatenate([case[0][:4], case[0][7:]])
    case[1]["samples"] = 6


@pytest.mark.parametrize("spoil", [_flip, _apart, _missing, _one_more, _samples, _decisions, _simulations, _empty])
def test_assert_streams_refuses(spoil):
    case = list(_case())
    spoil(case)
    with pytest.raises(AssertionError):
        SR.assert_streams(*case)


def test_outcome_z():
    assert [SR.outcome_z(1, 1), SR.outcome_z(1, 0), SR.outcome_z(0, 0), SR.outcome_z(-2, 0), SR.outcome_z(-2, 1)] == [1.0, -1.0, 1.0, 0.0, 0.0]


def test_equal_runs_share_a_cache_slot(monkeypatch):
    a = SR.Run(9100, 4, 2, 8, fast=4, cap=(0.5, 99), dirichlet=(0.3, 77), forced=(2.0, True), surprise=(0.75, 4.0, 31))
    b = SR.Run(9100, 4, 2, 8, fast=4, cap=(0.5, 99), dirichlet=(0.3, 77), forced=(2.0, True), surprise=(0.75, 4.0, 31))
    assert a == b and hash(a) == hash(b) and a is not b and a != a._replace(value_mix=0.5)
    calls = []
    monkeypatch.setattr(SR, "_cache", {})
    monkeypatch.setattr(SR, "retrace", lambda run: calls.append(run) or ("games", len(calls)))
    first = SR.cached("retrace", a)
    assert SR.cached("retrace", b) is first and len(calls) == 1
    assert SR.cached("retrace", a._replace(value_mix=0.5, surprise=None)) is first and len(calls) == 1   # the retrace does not look at them
    assert SR.cached("retrace", a._replace(threads=1)) is not first and len(calls) == 2
