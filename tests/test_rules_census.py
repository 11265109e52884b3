"""CPU: the inputs of the lock-step tests off the default settings (tests/test_gpu_rules.py::test_lockstep_random_games_under_settings)
reach every branch they are meant to compare.  Counted on the oracle's games alone, by tests/rules_settings.py."""
import pytest

import rules_settings as RS


@pytest.mark.parametrize("kw", RS.SETTINGS, ids=RS.setting_id)
def test_each_setting_reaches_its_situations(orc, kw):
    count = RS.census(kw)
    short = {k: count[k] for k in RS.required(kw) if count[k] < RS.CENSUS_MIN}
    assert not short, (short, count)
    assert len(RS.oracle_games(kw)) == len(RS.seeds(kw)) >= RS.GAMES
    assert all(g["status"] != -1 for g in RS.oracle_games(kw))   # every game was played to its end


def test_every_situation_is_required_somewhere():
    asked = set().union(*(RS.required(kw) for kw in RS.SETTINGS))
    assert asked == set(RS.SITUATIONS)
    for k in RS.LONG_GAME_ONLY:   # the saturated ones in both long settings
        assert k in RS.required(RS.LONG) and k in RS.required(RS.FIVE)


def test_the_classifier_on_hand_made_states(orc):
    """the census counts what it says: states written by hand"""
    import ctypes as C

    import azr_testlib as T
    s = T.OrcState()
    orc.orc_state_blank(C.byref(s))
    s.cur = 0
    for l in range(42):
        s.owner[l], s.army[l] = 1, 1
    nb = RS.neighbours()
    t = 0
    a, b = nb[t][0], nb[t][1]
    for l, n in ((t, 32), (a, 5), (b, 5)):
        s.owner[l], s.army[l] = 0, n
    s.phase = RS.PH_FORTIFY
    assert RS.classify(s, 0, t, {}) == ["fortify_target_full"]
    s.army[t] = 30
    assert sorted(RS.classify(s, 0, t, {})) == ["fortify_clamped", "fortify_source_tie"]
    s.army[b] = 2
    assert sorted(RS.classify(s, 0, t, {})) == [
        "fortify_clamped", "fortify_source_unique"]
    s.army[t] = 3
    assert RS.classify(s, 0, t, {}) == ["fortify_source_unique"]
    s.phase = RS.PH_ATTACK
    s.owner[t], s.army[b] = 1, 5
    assert RS.classify(s, 0, t, {}) == ["attack_source_tie"]
    s.army[b] = 6
    assert RS.classify(s, 0, t, {}) == ["attack_source_unique"]
    s.phase, s.mob_from, s.mob_to = RS.PH_MOBILIZATION, b, t
    assert RS.classify(s, 0, t, dict(min_unit_move=2)) == ["mobilize_half"]      # value 5, 5 // 2 >= 2
    assert RS.classify(s, 0, t, {}) == ["mobilize_min_unit"]                    # 5 // 2 < 3 <= 5
    assert RS.classify(s, 0, t, dict(min_unit_move=6)) == ["mobilize_all"]       # 5 < 6
    assert RS.classify(s, 0, b, {}) == []                                       # the stop, no move
    s.phase, s.reinf, s.army[a] = RS.PH_REINFORCEMENT, 9, 30
    assert RS.classify(s, 0, a, {}) == ["reinforce_clamped"]                    # wants 4, room for 2
    assert RS.classify(s, 0, b, {}) == []
    assert RS.classify(s, 1 << 42, 42, {}) == ["reinforce_skip_only"] and RS.classify(s, (1 << 42) | 1, 42, {}) == []
    s.ps[0].cards, s.card_sets = 3, 6
    assert "card_set_7_up" in RS.classify(s, 0, b, {})
    s.card_sets = 5
    assert "card_set_7_up" not in RS.classify(s, 0, b, {})
    s.round = 59
    assert RS.classify_end(s, 1, {}) == [] and RS.classify_end(s, 1, dict(allow_yield=0)) == ["round_limit_end"]   # 3 lands to 39
    assert RS.classify_end(s, -2, dict(allow_yield=0)) == ["draw", "round_limit_end"]
