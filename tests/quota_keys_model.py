"""Test infrastructure only -- the path from a Quota request to memquota's HandleQuota, restated on
top of oracle.memquota.Memquota and tests/quota_dedup_model.py:

  makeKey          mixer/adapter/memquota/keys.go:35-95
  matchDimensions  memquota.go:65-85
  limit            memquota.go:87-105
  HandleQuota      memquota.go:107-116
  dispatch         mixer/pkg/runtime/dispatcher.go:242-281, :160-187 (the first rule with a quota
                   action dispatches that action's first instance, nothing else)
  response         mixer/pkg/api/grpcServer.go:188-257

Dimension values are Python values standing for what Result.AsInterface returns (result.go:96-116):
str -> string, int -> int64, float -> float64, bool -> bool, bytes -> []byte, dict -> map[string]string;
any other object with a String() method is a fmt.Stringer (net.IP, time.Duration, time.Time).
EvalError marks a label whose Eval failed; Unsupported a run-time kind outside the device's v1 scope.

Key ids, classes and the conflict rule are the product's own (include/mxp.h mxp_quota_batch): a class
is a (limit, default) or (limit, override) pair owning the id range [base, base + key_cap); a call's
new keys of a class take its next free ids in order of first arrival; a key text held under another
class is a conflict.
"""
from __future__ import annotations

import struct

import memquota as M  # noqa: F401  (oracle/ on sys.path: the importer's business, as for quota_dedup_model)
from quota_dedup_model import DedupQuota

OK, NOT_APPLIED, OTHER, SKIPPED, RESOLVE_ERROR = 0, 1, 2, 3, 4
EVAL_ERROR, KEY_UNSUPPORTED, KEYS_FULL, KEY_CONFLICT = -1, -2, -3, -4
NO_UNIT, OTHER_UNIT = 0xFFFFFFFF, 0xFFFFFFFE
NO_KEY = 0xFFFFFFFF
PAD = b"\0" * 32  # keys.go appends to bytes[:] of a [32]byte: a slice of length 32


class EvalError:
    """a dimension whose Eval failed"""


class Unsupported:
    """a run-time kind the device stage refuses (DURATION, TIMESTAMP, STRING_MAP)"""


def format_int_hex(v: int) -> bytes:
    """strconv.AppendInt(v, 16)"""
    return (b"-" if v < 0 else b"") + b"%x" % abs(v)


def format_float_b(x: float) -> bytes:
    """strconv.AppendFloat(x, 'b', -1, 64) (ftoa.go genericFtoa, fmtB), from the bits"""
    bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    return format_bits_b(bits)


def format_bits_b(bits: int) -> bytes:
    neg, exp, mant = bits >> 63, (bits >> 52) & 0x7FF, bits & ((1 << 52) - 1)
    if exp == 0x7FF:
        return b"NaN" if mant else (b"-Inf" if neg else b"+Inf")
    if exp == 0:
        exp = 1
    else:
        mant |= 1 << 52
    exp += -1023 - 52
    return (b"-" if neg else b"") + b"%d" % mant + b"p" + (b"+" if exp >= 0 else b"") + b"%d" % exp


def value_bytes(v) -> bytes:
    if isinstance(v, str):
        return v.encode("utf-8", "surrogateescape")
    if isinstance(v, bool):  # (before int: Python's bool is an int)
        return PAD + (b"true" if v else b"false")
    if isinstance(v, int):
        return PAD + format_int_hex(v)
    if isinstance(v, float):
        return PAD + format_float_b(v)
    if isinstance(v, (bytes, bytearray)):
        return bytes(v)
    if isinstance(v, dict):
        return b"".join(value_bytes(k) + value_bytes(v[k]) for k in sorted(v))
    return value_bytes(v.String())


def make_key(name: str, labels: dict) -> bytes:
    out = value_bytes(name)
    for k in sorted(labels):  # sort.Strings: byte order, as Python's for these ASCII labels
        out += b";" + value_bytes(k) + b"=" + value_bytes(labels[k])
    return out


def match_dimensions(cfg: dict, inst: dict) -> bool:
    for k, val in cfg.items():
        rval = inst.get(k)
        if isinstance(rval, str) and rval == val:  # rval == val on interfaces: a string equal to it
            continue
        if hasattr(rval, "String") and rval.String() == val:
            continue
        return False
    return True


def limit(cfg: dict, dims: dict):
    """cfg: {"max_amount", "valid_duration_ns", "overrides": [{"dimensions", "max_amount",
    "valid_duration_ns"}]} -> (override index or -1, the Limit)."""
    for i, o in enumerate(cfg.get("overrides", ())):
        if match_dimensions(o.get("dimensions", {}), dims):
            return i, o
    return -1, cfg


def dispatch(status: int, rules, rule_unit):
    """-> (code, unit): RESOLVE_ERROR / NOT_APPLIED / OTHER, or (OK, unit index)"""
    if status != 0:
        return RESOLVE_ERROR, None
    for r in rules:
        u = rule_unit[r]
        if u == NO_UNIT:
            continue
        if u == OTHER_UNIT:
            return OTHER, None
        return OK, u
    return NOT_APPLIED, None


class QuotaPlanModel:
    """limits: [{"name", "max_amount", "valid_duration_ns", "key_cap", "overrides": [{"dimensions",
    "max_amount", "valid_duration_ns", "key_cap"}]}]; units: [{"instance_name", "labels"}]."""

    def __init__(self, limits, units, rule_unit, default_valid_ns=10 * 10**9):
        self.limits, self.units, self.rule_unit, self.default_valid_ns = limits, units, list(rule_unit), default_valid_ns
        self.by_name = {lim["name"]: i for i, lim in enumerate(limits)}
        self.class_base, self.class_cap, self.class_limit = {}, {}, {}
        base, expanded = 0, {}
        for li, lim in enumerate(limits):
            for oi, c in [(-1, lim)] + list(enumerate(lim.get("overrides", ()))):
                self.class_base[li, oi], self.class_cap[li, oi] = base, c["key_cap"]
                for k in range(c["key_cap"]):
                    expanded[base + k] = (c["max_amount"], c["valid_duration_ns"])
                base += c["key_cap"]
        self.n_keys = base
        self.expanded = expanded  # id -> (max_amount, valid_duration_ns): mxp_quota_create's arrays
        self.next_free = {c: 0 for c in self.class_base}
        self.table = {}   # key bytes -> (class, id)
        self.text = {}    # id -> key bytes
        self.dq = DedupQuota(expanded)

    def stage(self, unit_of, dims_of, amounts):
        """The key stage of one call: per request (code, key id, failed mask, key bytes or None).
        unit_of[q]: a unit index or None (not HandleQuota's); dims_of(q, unit) -> {label: value}."""
        n = len(amounts)
        out = [None] * n
        pending = {}  # key bytes -> (class, [requests]) of this call's new keys, in first-arrival order
        for q in range(n):
            u = unit_of[q]
            if u is None:
                continue
            unit = self.units[u]
            dims = dims_of(q, u)
            failed = 0
            for j, lab in enumerate(unit["labels"]):
                if isinstance(dims[lab], EvalError) or dims[lab] is EvalError:
                    failed |= 1 << j
            if failed:
                out[q] = (EVAL_ERROR, NO_KEY, failed, None)
                continue
            if any(isinstance(v, Unsupported) or v is Unsupported for v in dims.values()):
                out[q] = (KEY_UNSUPPORTED, NO_KEY, 0, None)
                continue
            if amounts[q] == 0:  # QuotaResult{}: no key is made
                out[q] = (OK, NO_KEY, 0, None)
                continue
            li = self.by_name[unit["instance_name"]]
            oi, _ = limit(self.limits[li], dims)
            key = make_key(unit["instance_name"], dims)
            held = self.table.get(key)
            if held is not None:
                out[q] = (OK, held[1], 0, key) if held[0] == (li, oi) else (KEY_CONFLICT, NO_KEY, 0, key)
                continue
            if key in pending:
                if pending[key][0] == (li, oi):
                    pending[key][1].append(q)
                else:
                    out[q] = (KEY_CONFLICT, NO_KEY, 0, key)
                continue
            pending[key] = ((li, oi), [q])
        for key, (c, reqs) in pending.items():  # (insertion order: first arrival)
            if self.next_free[c] >= self.class_cap[c]:
                for q in reqs:
                    out[q] = (KEYS_FULL, NO_KEY, 0, key)
                continue
            kid = self.class_base[c] + self.next_free[c]
            self.next_free[c] += 1
            self.table[key] = (c, kid)
            self.text[kid] = key
            for q in reqs:
                out[q] = (OK, kid, 0, key)
        return out

    def batch(self, status, rules_of, dims_of, amounts, best_effort, ids, skip, now_ns):
        """mxp_quota_batch -> per request (granted, valid_ns, key, code, dup, failed & 255).
        ids: per-request DeduplicationID bytes, or None (no dedup); skip: flags or None."""
        n = len(amounts)
        early, unit_of = [None] * n, [None] * n
        for q in range(n):
            if skip is not None and skip[q]:
                early[q] = SKIPPED
            else:
                code, u = dispatch(int(status[q]), rules_of(q), self.rule_unit)
                if code == OK:
                    unit_of[q] = u
                else:
                    early[q] = code
        st = self.stage(unit_of, dims_of, amounts)
        out = []
        for q in range(n):
            a = int(amounts[q])
            if early[q] is not None:
                g, v = (a, self.default_valid_ns) if early[q] == NOT_APPLIED else (0, 0)
                out.append((g, v, NO_KEY, early[q], 0, 0))
                continue
            code, kid, failed, _ = st[q]
            if code != OK or kid == NO_KEY:
                out.append((0, 0, NO_KEY, code, 0, failed & 255))
                continue
            if ids is None:
                g = self.dq.q.handle(kid, a, bool(best_effort[q]), now_ns)
                vd = self.expanded[kid][1]
                v = vd if a > 0 and vd != 0 and (best_effort[q] or g > 0) else 0
                dup = 0
            else:
                g, v, dup, _ = self.dq.handle(kid, a, bool(best_effort[q]), ids[q], now_ns)
            out.append((g, v, kid, OK, dup, 0))
        return out
