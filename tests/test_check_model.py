"""tests/check_model.py pinned on hand-derived rows: the reference's TestCheck rows
(tests/golden/dispatcher_check.json, transcribed from mixer/pkg/runtime/dispatcher_test.go:121-123)
and one row per quirk of combineResults / grpcServer.Check the batched Check reproduces.  Every
expected tuple is written out here: (valid_duration_ns, valid_use_count, code, n_records, flags)."""
import json
import os

import check_model as M

S = 10 ** 9
DEF = M.DEFAULTS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatcher_check.json")


def run(status, rules, rule_units, units):
    """units: {unit: (code, duration, use count, value)}"""
    return M.check_request(status, rules, rule_units, lambda u: units[u])


def test_reference_testcheck_rows():
    g = json.load(open(GOLDEN))
    handlers = g["handlers"]
    assert len(g["rows"]) == 3
    for row in g["rows"]:
        c = row["call"]
        assert row["ncalled"] == 6 == len(handlers)
        # three actions (rules 0, 1, 2) of two instances each: units 0..5, every call the same result
        rule_units = {0: [0, 1], 1: [2, 3], 2: [4, 5]}
        units = {u: (c["code"], c["valid_duration_ns"], c["valid_use_count"], 0) for u in range(6)}
        res, recs = run(0, [0, 1, 2], rule_units, units)
        w = row["want"]
        assert res[:3] == (w["valid_duration_ns"], w["valid_use_count"], w["code"])
        assert res[3] == len(recs) == (6 if c["code"] else 0)
        assert M.message(recs, lambda u: handlers[u], lambda u, code, v: c["message"]) == w["message"]
    # (the third row, spelled out: PERMISSION_DENIED "bad user" six times)
    assert res == (0, 200, 7, 6, 0)
    assert [r[:3] for r in recs] == [(0, 0, 7), (0, 1, 7), (1, 2, 7), (1, 3, 7), (2, 4, 7), (2, 5, 7)]


def test_eval_error_alone_is_ok_0_0():
    """ProcessCheck returned CheckResult{} and an error: the zero result is the combination, and
    out = cr.Status = OK."""
    res, recs = run(0, [4], {4: [0]}, {0: (M.EVAL_ERROR, 3 * S, 50, 0)})
    assert res == (0, 0, 0, 1, M.F_EVAL_ERROR)
    assert recs == [(4, 0, -1, 0)]


def test_eval_error_after_not_found_keeps_the_code():
    res, recs = run(0, [1, 2], {1: [0], 2: [1]}, {0: (5, 3 * S, 50, 77), 1: (M.EVAL_ERROR, 9 * S, 9, 0)})
    assert res == (0, 0, 5, 2, M.F_EVAL_ERROR)
    assert recs == [(1, 0, 5, 77), (2, 1, -1, 0)]


def test_panic_alone_is_internal_with_defaults():
    res, recs = run(0, [3], {3: [0]}, {0: (M.NOT_STRING, 3 * S, 50, 0)})
    assert res == (10 * S, 200, 13, 1, M.F_UNIT_PANIC | M.F_NO_CHECKS)
    assert recs == [(3, 0, -2, 0)]


def test_panic_beside_an_ok_result_changes_nothing():
    res, recs = run(0, [3], {3: [0, 1]}, {0: (M.NOT_STRING, 1 * S, 1, 0), 1: (0, 3 * S, 50, 0)})
    assert res == (3 * S, 50, 0, 1, M.F_UNIT_PANIC)
    assert recs == [(3, 0, -2, 0)]


def test_resolve_error_is_internal_with_defaults():
    for status in (1, 2, 3):
        res, recs = run(status, [], {}, {})
        assert res == (10 * S, 200, 13, 0, M.F_RESOLVE_ERROR) and recs == []
    assert DEF == (10 * S, 200)


def test_nothing_selected_is_ok_with_defaults():
    assert run(0, [], {}, {}) == ((10 * S, 200, 0, 0, M.F_NO_CHECKS), [])
    # (selected rules without units: the same)
    assert run(0, [5, 6], {5: [], 6: []}, {}) == ((10 * S, 200, 0, 0, M.F_NO_CHECKS), [])


def test_two_failures_first_code_both_parts():
    units = {0: (0, 5 * S, 500, 0), 1: (7, 4 * S, 400, 11), 2: (5, 6 * S, 300, 22)}
    res, recs = run(0, [9, 2], {9: [0, 1], 2: [2]}, units)
    assert res == (4 * S, 300, 7, 2, 0)
    assert recs == [(9, 1, 7, 11), (2, 2, 5, 22)]
    names = {1: "deny", 2: "allow"}
    sym = {11: "eve", 22: "bob"}
    text = M.message(recs, names.get, lambda u, c, v: M.list_message(c, sym[v]))
    assert text == "deny:eve is blacklisted, allow:bob is not whitelisted"
    # (the other order of the same rules: the other code first)
    res, recs = run(0, [2, 9], {9: [0, 1], 2: [2]}, units)
    assert res == (4 * S, 300, 5, 2, 0) and [r[1] for r in recs] == [2, 1]


def test_duration_min_is_64_bit():
    """10 s = 0x2_540B_E400 ns against 3 s = 0x0_B2D0_5E00 ns: the low half of 10 s is the smaller one,
    so a min per 32-bit half would answer 0x0_540B_E400."""
    assert (10 * S) & 0xFFFFFFFF < (3 * S) & 0xFFFFFFFF
    res, _ = run(0, [0], {0: [0, 1]}, {0: (0, 10 * S, 7, 0), 1: (0, 3 * S, 9, 0)})
    assert res == (3 * S, 7, 0, 0, 0)
    res, _ = run(0, [0], {0: [0, 1]}, {0: (0, 1 << 40, 7, 0), 1: (0, 10 * S, -3, 0)})
    assert res == (10 * S, -3, 0, 0, 0)
    # (signed: a negative duration is the minimum)
    res, _ = run(0, [0], {0: [0, 1]}, {0: (0, -1, 7, 0), 1: (0, 3 * S, 9, 0)})
    assert res[:2] == (-1, 7)
