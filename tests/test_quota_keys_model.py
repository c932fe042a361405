"""tests/quota_keys_model.py against the reference's own rows (tests/golden/memquota_keys.json:
TestHandler_Limit, the TestAllocAndRelease dimension map with its key written out by hand, float and
int known answers), and its own dispatch / id / conflict rules on small hand-made cases."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)

import quota_keys_model as Q  # noqa: E402

with open(os.path.join(HERE, "golden", "memquota_keys.json")) as f:
    GOLD = json.load(f)


class NetIP:
    """stands in for net.IP: a fmt.Stringer that is no string"""

    def __init__(self, text):
        self.text = text

    def String(self):
        return self.text


def decode(v):
    (kind, x), = v.items() if isinstance(v, dict) else (("string", v),)
    if kind == "net.IP":
        return NetIP(x)
    if kind == "float64_bits":
        import struct
        return struct.unpack("<d", struct.pack("<Q", int(x, 16)))[0]
    if kind == "bytes_hex":
        return bytes.fromhex(x)
    return x  # string, int64, bool, map


@pytest.mark.parametrize("row", GOLD["limit_rows"], ids=lambda r: r["desc"])
def test_handler_limit_rows(row):
    inst = {k: decode(v) for k, v in row["inst"].items()}
    _, lim = Q.limit(row["cfg"], inst)
    assert lim["max_amount"] == row["limit"]


def test_ip_as_bytes_does_not_match():
    """[]byte is neither a string nor a Stringer (memquota.go:69-80); nor are int64, float64, bool"""
    row = GOLD["limit_rows"][3]
    import ipaddress
    raw = ipaddress.ip_address("192.10.1.118").packed
    assert Q.limit(row["cfg"], {"source.ip": raw})[0] == -1
    assert Q.limit(row["cfg"], {"source.ip": NetIP("192.10.1.118")})[0] == 0
    assert Q.limit(row["cfg"], {})[0] == -1  # a label the instance lacks
    cfg = {"max_amount": 1, "overrides": [{"dimensions": {"a": "2"}, "max_amount": 2}]}
    for v in (2, 2.0, True, b"2"):
        assert Q.limit(cfg, {"a": v})[0] == -1
    assert Q.limit(cfg, {"a": "2"})[0] == 0


def test_alloc_and_release_key():
    g = GOLD["alloc_and_release_key"]
    dims = {k: decode(v) for k, v in g["dims"].items()}
    want = g["key"].encode("latin-1")
    assert want.count(b"\0" * 32) == 3
    assert Q.make_key(g["name"], dims) == want


def test_known_answers():
    for bits, text in GOLD["float_b"]:
        assert Q.format_bits_b(int(bits, 16)) == text.encode(), bits
    for v, text in GOLD["int_hex"]:
        assert Q.format_int_hex(v) == text.encode(), v
    assert Q.format_float_b(1.0) == b"4503599627370496p-52"  # (strconv's own documented example)
    assert Q.value_bytes(True) == Q.PAD + b"true" and Q.value_bytes(False) == Q.PAD + b"false"
    assert Q.value_bytes(1) == Q.PAD + b"1"  # (an int, not the bool)


def test_key_text_is_not_injective():
    a = Q.make_key("q", {"a": "x;b=y", "b": "z"})
    b = Q.make_key("q", {"a": "x", "b": "y;b=z"})
    assert a == b == b"q;a=x;b=y;b=z"


def test_dispatch_walk():
    ru = [Q.NO_UNIT, 1, Q.OTHER_UNIT, 0]
    assert Q.dispatch(1, [1], ru) == (Q.RESOLVE_ERROR, None)
    assert Q.dispatch(0, [], ru) == (Q.NOT_APPLIED, None)
    assert Q.dispatch(0, [0, 0], ru) == (Q.NOT_APPLIED, None)
    assert Q.dispatch(0, [0, 3, 1], ru) == (Q.OK, 0)       # the first rule with a unit, nothing else
    assert Q.dispatch(0, [0, 2, 1], ru) == (Q.OTHER, None)  # another handler's, ahead of ours
    assert Q.dispatch(0, [1, 2], ru) == (Q.OK, 1)


LIMITS = [{"name": "rq", "max_amount": 5, "valid_duration_ns": 0, "key_cap": 3,
           "overrides": [{"dimensions": {"a": "x"}, "max_amount": 9, "valid_duration_ns": 10**9, "key_cap": 2}]}]
UNITS = [{"instance_name": "rq", "labels": ["a", "b"]}]


def run(plan, dims, amounts, ids=None, skip=None, now=10**18):
    n = len(dims)
    return plan.batch([0] * n, lambda q: [0], lambda q, u: dims[q], amounts, [0] * n, ids, skip, now)


def test_ids_capacity_and_persistence():
    p = Q.QuotaPlanModel(LIMITS, UNITS, [0])
    assert p.n_keys == 5 and p.expanded[0] == (5, 0) and p.expanded[3] == (9, 10**9)
    dims = [{"a": "p%d" % (i % 5), "b": "v"} for i in range(7)]
    out = run(p, dims, [1] * 7)
    assert [o[3] for o in out] == [0, 0, 0, Q.KEYS_FULL, Q.KEYS_FULL, 0, 0]
    assert [o[2] for o in out] == [0, 1, 2, Q.NO_KEY, Q.NO_KEY, 0, 1]
    assert [o[0] for o in out] == [1, 1, 1, 0, 0, 1, 1]
    again = run(p, dims, [1] * 7)
    assert [(o[2], o[3]) for o in again] == [(o[2], o[3]) for o in out]
    # the override's class has ids of its own; amount 0 interns nothing
    out = run(p, [{"a": "x", "b": "1"}, {"a": "x", "b": "2"}, {"a": "x", "b": "1"}], [0, 4, 4])
    assert [(o[2], o[3], o[0], o[1]) for o in out] == [(Q.NO_KEY, 0, 0, 0), (3, 0, 4, 10**9), (4, 0, 4, 10**9)]
    assert p.text[3] == b"rq;a=x;b=2"


def test_conflict_eval_error_unsupported_and_early_codes():
    p = Q.QuotaPlanModel(LIMITS, UNITS, [0, Q.NO_UNIT, Q.OTHER_UNIT], default_valid_ns=7)
    dims = [{"a": "x;b=y", "b": "z"}, {"a": "x", "b": "y;b=z"}, {"a": Q.EvalError, "b": Q.EvalError},
            {"a": "k", "b": Q.Unsupported}, {"a": "k", "b": Q.EvalError}]
    out = run(p, dims, [2, 2, 2, 2, 2])
    assert out[0][2:4] == (0, Q.OK) and out[1][2:4] == (Q.NO_KEY, Q.KEY_CONFLICT) and out[1][0] == 0
    assert out[2][3] == Q.EVAL_ERROR and out[2][5] == 3 and out[4][5] == 2 and out[3][3] == Q.KEY_UNSUPPORTED
    assert p.dq.q.cells == {0: 2}  # (no state moved for anyone else)
    rules = [[1], [1, 2, 0], [0], []]
    out = p.batch([0, 0, 1, 0], lambda q: rules[q], lambda q, u: {"a": "k", "b": "k"}, [3, 3, 3, 3], [0] * 4, None,
                  [0, 0, 0, 1], 0)
    assert [o[3] for o in out] == [Q.NOT_APPLIED, Q.OTHER, Q.RESOLVE_ERROR, Q.SKIPPED]
    assert out[0][:2] == (3, 7) and out[1][:2] == (0, 0)


def test_quota_instance_workload_names_its_keys():
    """workloads.quota_instance_workload: the four dimensions spell exactly the drawn key indices, an
    eighth of the keys (fewer of the requests: Zipf favours keys 0 .. 31) fall under the override,
    ids repeat."""
    from istio_amd import workloads as W
    w = W.quota_instance_workload(n_rules=40, n_requests=3000, n_keys=1024, seed=6)
    b = w["batch"]
    lim, unit = w["limits"][0], w["units"][0]
    texts, over = {}, 0
    for q in range(b.n):
        dims = {lab: b.get(q, w["inst_rules"][r])[0] for lab, r in zip(unit["labels"], unit["value_rules"])}
        assert all(isinstance(v, str) for v in dims.values())
        k = int(w["key_index"][q])
        assert texts.setdefault(Q.make_key(unit["instance_name"], dims), k) == k
        over += Q.limit(lim, dims)[0] == 0
    assert len(texts) == len(set(w["key_index"].tolist())) > 300
    assert 0.03 * b.n < over < 0.3 * b.n
    assert len(set(w["ids"])) < b.n and (w["amounts"] == 0).any() and (w["amounts"] < 0).any()
    assert sum(1 for m in w["conf"]["variety_mask"] if m >> W.QUOTA_VARIETY & 1) == 10
    assert [u == 0 for u in w["rule_unit"]] == [bool(m >> W.QUOTA_VARIETY & 1) for m in w["conf"]["variety_mask"]]


def test_dedup_hits_intern_their_key():
    p = Q.QuotaPlanModel(LIMITS, UNITS, [0])
    dims = [{"a": "1", "b": "1"}, {"a": "2", "b": "2"}]
    out = run(p, dims, [1, 1], ids=[b"same", b"same"])
    assert [(o[2], o[4], o[0]) for o in out] == [(0, 0, 1), (1, 1, 1)]  # the follower's key has its id
    assert p.dq.q.cells == {0: 1}
