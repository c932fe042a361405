"""The device half of IP_ADDRESSES lists (mxp_list_create's tables, lists.hip find4 / find4_dir /
le128 / ip_member, the family regroup of mxp_list_ip_kernel) against the independent reference of
tests/test_cidr_independent.py: the same lists and lookups, expected codes from that reference --
not from the oracle -- through every path (MXP_LIST_IP_SPLIT x MXP_LIST_OPT), whitelist and
blacklist.  The codes are integers: the bar is equality."""
import numpy as np
import pytest

import lists as L
from test_cidr_independent import (GO_ONLY_ENTRIES, GO_ONLY_LOOKUPS, INVALID, MALFORMED, RefList, cases, parse_error,
                                   ref_addr)

pytestmark = pytest.mark.gpu

# MXP_LIST_IP_SPLIT (the family regroup on / off) x MXP_LIST_OPT (255 all on, 0 all off, 1 the
# register parse, 2 the /16 directory, 3 both)
PATHS = [(split, opt) for split in ("1", "0") for opt in ("255", "0", "1", "2", "3")]
COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)


@pytest.fixture(scope="module")
def eng(libmxp):
    import istio_amd.engine as mxp
    return mxp.Engine(0)


@pytest.fixture(scope="module")
def gpu_lists(eng):
    return [eng.list_create(L.IP_ADDRESSES, c.entries, c.overrides) for c in cases()]


def _set_path(monkeypatch, split, opt):
    monkeypatch.setenv("MXP_LIST_IP_SPLIT", split)
    monkeypatch.setenv("MXP_LIST_OPT", opt)


def _same(lst, lookups, found, what):
    for black in (False, True):
        want = L.codes(found, black)
        got = lst.check(lookups, black)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, black, [(lookups[i], int(got[i]), int(want[i])) for i in bad[:8]])


def test_num_entries_and_parse_errors(eng, gpu_lists):
    from istio_amd.engine import MxpError
    for c, lst in zip(cases(), gpu_lists):
        assert lst.num_entries() == c.ref.n_entries, c.name
    for e in MALFORMED:
        with pytest.raises(MxpError) as ei:
            eng.list_create(L.IP_ADDRESSES, ["10.0.0.0/8", e, "11.0.0.0/8"], [])
        assert str(ei.value).endswith(parse_error(e)), (e, str(ei.value))
    # the same entries as overrides: skipped without error, not counted
    lst = eng.list_create(L.IP_ADDRESSES, ["10.0.0.0/8"], MALFORMED + ["11.0.0.0/8"])
    assert lst.num_entries() == 2
    assert list(lst.check(["10.1.1.1", "11.1.1.1", "12.1.1.1"])) == [L.OK, L.OK, L.NOT_FOUND]


@pytest.mark.parametrize("split,opt", PATHS)
def test_lists_agree_with_reference(gpu_lists, monkeypatch, split, opt):
    """Every list of the CPU module -- the fixed edge tables, the seeded lists of 1, 3, 40 and 1,000
    entries -- with its lookups (interval bounds and their neighbours, both spellings of IPv4
    values, one-word differences of IPv6 bounds, random and invalid strings)."""
    _set_path(monkeypatch, split, opt)
    for c, lst in zip(cases(), gpu_lists):
        _same(lst, c.lookups, c.want, c.name)


def _pools(c):
    """A case's lookups by what mxp_list_ip_kernel makes of their first 8 bytes: '.' first (the
    IPv4 lanes), the other valid ones (IPv6 and 4-in-6), and invalid non-empty strings."""
    v4 = [s for s in c.lookups if ref_addr(s) is not None and ":" not in s]
    v6 = [s for s in c.lookups if ref_addr(s) is not None and ":" in s]
    bad = [s for s in INVALID if s] + [s for s in c.lookups if s and ref_addr(s) is None]
    assert len(v4) >= 30 and len(v6) >= 30 and len(bad) >= 30
    take = lambda pool, n: [pool[i % len(pool)] for i in range(n)]  # noqa: E731
    return take, v4, v6, bad


@pytest.mark.parametrize("split,opt", PATHS)
def test_regroup_shapes(gpu_lists, monkeypatch, split, opt):
    """The regroup of a workgroup's lanes by family at the shapes where it can go wrong: lookup
    counts around one wave and one workgroup, and workgroups (256 lookups) of one family only, of
    invalid strings only, of empty strings only, split 128 / 128, with a single lane of the other
    family, and a last workgroup of one lane."""
    _set_path(monkeypatch, split, opt)
    for name in ("edge-both", "gen-1000"):
        c, lst = next((c, g) for c, g in zip(cases(), gpu_lists) if c.name == name)
        take, v4, v6, bad = _pools(c)
        for n in COUNTS:
            _same(lst, c.lookups[:n], c.want[:n], (name, n))
        blocks = {"v4": take(v4, 256), "v6": take(v6, 256), "invalid": take(bad, 256), "empty": [""] * 256,
                  "half": take(v4, 128) + take(v6, 128), "mixed": [x for p in zip(take(v4, 128), take(v6, 128)) for x in p],
                  "one-v6": take(v4, 100) + take(v6, 1) + take(v4, 155), "one-v4": take(v6, 255) + take(v4, 1),
                  "one-valid": [""] * 255 + take(v6, 1)}
        for k, b in blocks.items():
            assert len(b) == 256
            _same(lst, b, c.ref.found(b), (name, k))
        whole = [s for b in blocks.values() for s in b] + take(v4, 1)  # ... and a last workgroup of one lane
        assert len(whole) % 256 == 1
        _same(lst, whole, c.ref.found(whole), (name, "all blocks"))
        whole = whole[:-1] + take(v6, 1)
        _same(lst, whole, c.ref.found(whole), (name, "all blocks, IPv6 last"))


@pytest.mark.parametrize("split", ["1", "0"])
def test_fused_listentry_first_workgroup_settled(eng, gpu_lists, monkeypatch, split):
    """mxp_listentry_check on 600 requests: requests 0..255 carry no attribute, so every lane of the
    first workgroup is settled with the eval-error code before the regroup; the rest carry the edge
    lookups.  Expected codes from the reference, -1 for the errors."""
    import istio_amd.engine as mxp
    from istio_amd.bags import BagBatch
    monkeypatch.setenv("MXP_LIST_IP_SPLIT", split)
    c, lst = next((c, g) for c, g in zip(cases(), gpu_lists) if c.name == "edge-both")
    addrs = [s for s in c.lookups if s and "\x00" not in s]
    addrs = [addrs[i % len(addrs)] for i in range(344)]
    bags = [{} for _ in range(256)] + [{"request.path": s} for s in addrs]
    manifest = {"request.path": "STRING"}
    batch = BagBatch.from_bags(bags, names=list(manifest))
    inst = mxp.Engine(0)
    inst.set_vocabulary(manifest)
    assert (inst.compile(["true", "request.path"]) == 0).all()
    found = c.ref.found(addrs)
    assert (found == 1).sum() > 50 and (found == 0).sum() > 50 and (found < 0).sum() > 3
    for black in (False, True):
        want = np.concatenate([np.full(256, -1, dtype=np.int32), L.codes(found, black)])
        got = lst.check_entries(inst, batch, 1, black)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (black, [(int(q), int(got[q]), int(want[q])) for q in bad[:8]])
    inst.close()


@pytest.mark.parametrize("split,opt", PATHS)
def test_go_only_spellings_gpu_equals_oracle(eng, monkeypatch, split, opt):
    """No expected value (Go 1.9 accepts leading zeros, `ipaddress` does not): the GPU agrees with the
    oracle.  `000000001.2.3.4` is a valid quad whose first "." lies past byte 8, which
    mxp_list_ip_kernel classifies as "other" from its first 8 bytes."""
    from istio_amd.engine import MxpError
    _set_path(monkeypatch, split, opt)
    base = ["10.0.0.0/8", "1.2.3.4", "2001:db8::/32", "1::/16"]
    ok = []
    for e in GO_ONLY_ENTRIES:
        try:
            L.IPList([e])
            ok.append(e)
        except L.ListParseError:
            with pytest.raises(MxpError):
                eng.list_create(L.IP_ADDRESSES, [e], [])
    o = L.IPList(base + ok)
    lst = eng.list_create(L.IP_ADDRESSES, base + ok, [])
    assert lst.num_entries() == o.num_entries()
    _same(lst, GO_ONLY_LOOKUPS, o.found(GO_ONLY_LOOKUPS, threads=1), "go-only")
    assert RefList(base).first_error is None
