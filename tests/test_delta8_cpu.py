"""MXP_RESOLVE_IDS_DELTA8 (include/mxp.h): the reference encoder and the decoder of the Python mirror
(istio_amd.engine.encode_delta8 / decode_delta8) against the format's worked vectors, round trips over
lists with every kind of step, and truncated streams."""
import numpy as np
import pytest

from istio_amd.engine import decode_delta8, encode_delta8

# (ids, bytes) as the header states them
VECTORS = [
    ([], ""),
    ([0], "00"),
    ([254], "FE"),
    ([255], "FF FF 00"),
    ([3, 4, 259, 10], "03 00 FE FF 0A 00"),
    ([0, 256], "00 FF 00 01"),
    ([65535], "FF FF FF"),
]


def enc_one(ids):
    boff, stream = encode_delta8([0, len(ids)], np.array(ids, dtype=np.uint16))
    assert boff.tolist() == [0, len(stream)]
    return stream


@pytest.mark.parametrize("ids,hexbytes", VECTORS)
def test_worked_vectors(ids, hexbytes):
    want = bytes.fromhex(hexbytes.replace(" ", ""))
    assert enc_one(ids).tobytes() == want
    off, back = decode_delta8([0, len(want)], np.frombuffer(want, dtype=np.uint8))
    assert off.tolist() == [0, len(ids)] and back.tolist() == ids and back.dtype == np.uint16


def test_vectors_concatenated():
    """requests are coded alone: a batch's stream is the concatenation of its requests' streams"""
    ids = [i for v, _ in VECTORS for i in v]
    off = np.cumsum([0] + [len(v) for v, _ in VECTORS])
    boff, stream = encode_delta8(off, ids)
    want = b"".join(bytes.fromhex(h.replace(" ", "")) for _, h in VECTORS)
    assert stream.tobytes() == want
    assert boff.tolist() == np.cumsum([0] + [len(bytes.fromhex(h.replace(" ", ""))) for _, h in VECTORS]).tolist()
    off2, ids2 = decode_delta8(boff, stream)
    assert off2.tolist() == off.tolist() and ids2.tolist() == ids


def random_lists(rng, n):
    """two ascending runs per request (one backward step), steps of exactly 254 / 255 / 256 (d + 1),
    first ids of at least 255, ids 0 and 65535, empty requests"""
    lists = []
    for q in range(n):
        kind = q % 8
        if kind == 0:
            lists.append([])
            continue

        def run(first, k):
            steps = rng.choice([1, 2, 26, 254, 255, 256, 257, 300, 1000], size=k,
                               p=[.3, .2, .2, .06, .06, .06, .04, .04, .04])
            r = first + np.concatenate([[0], np.cumsum(steps)])
            return r[r <= 65535]
        first = int(rng.integers(255, 40000)) if kind in (1, 2) else 0 if kind == 3 else int(rng.integers(0, 255))
        a = run(first, int(rng.integers(0, 90)))
        if kind == 4:
            a = np.concatenate([a[a < 65535], [65535]])
        b = run(int(rng.integers(0, max(1, int(a[0])))), int(rng.integers(0, 40)))  # starts below a: a backward step
        b = b[b < a[0]] if kind != 5 else b[:0]
        lists.append(np.concatenate([a, b]).tolist() if kind != 6 else np.concatenate([b, a]).tolist())
    return lists


def test_round_trip_random():
    rng = np.random.default_rng(8)
    lists = random_lists(rng, 4000)
    off = np.cumsum([0] + [len(x) for x in lists])
    ids = np.array([i for x in lists for i in x], dtype=np.uint16)
    # the cases are there
    d = np.diff(ids.astype(np.int64))
    assert any(len(x) == 0 for x in lists) and any(x and x[0] >= 255 for x in lists)
    assert {253, 254, 255} <= set((d - 1).tolist()) and ids.min() == 0 and ids.max() == 65535
    assert sum(1 for x in lists if np.any(np.diff(x) < 0)) > 1000
    assert max(int(np.sum(np.diff(x) < 0)) for x in lists if len(x) > 1) == 1
    boff, stream = encode_delta8(off, ids)
    assert boff[0] == 0 and boff[-1] == len(stream) and stream.dtype == np.uint8 and boff.dtype == np.uint64
    # against a plain per-id loop
    want = bytearray()
    wboff = [0]
    for x in lists:
        prev = -1
        for r in x:
            dd = r - prev - 1
            want += bytes([dd]) if 0 <= dd <= 254 else bytes([0xFF, r & 0xFF, r >> 8])
            prev = r
        wboff.append(len(want))
    assert stream.tobytes() == bytes(want) and boff.tolist() == wboff
    off2, ids2 = decode_delta8(boff, stream)
    assert np.array_equal(off2, off) and np.array_equal(ids2, ids)
    # a slice of the requests decodes alone
    off3, ids3 = decode_delta8(boff[100:301], stream)
    assert np.array_equal(off3, off[100:301] - off[100]) and np.array_equal(ids3, ids[off[100]:off[300]])


def test_runs_of_ff_bytes():
    """FF as an escape's id byte: the decoder may not take it for an escape"""
    lists = [[255, 65535, 255, 511], [0xFFFF], [0xFF, 0x1FF, 0x2FF, 0xFFFF, 0xFF], [], [0xFFFF, 0xFF]]
    off = np.cumsum([0] + [len(x) for x in lists])
    ids = [i for x in lists for i in x]
    boff, stream = encode_delta8(off, ids)
    off2, ids2 = decode_delta8(boff, stream)
    assert off2.tolist() == off.tolist() and ids2.tolist() == ids


@pytest.mark.parametrize("cut", [1, 2])
def test_truncated_escape_raises(cut):
    boff, stream = encode_delta8([0, 2, 3], [5, 600, 7])  # 05 FF 58 02 | 07
    assert stream.tobytes() == bytes([5, 0xFF, 0x58, 0x02, 7])
    with pytest.raises(ValueError):  # the stream ends inside the escape
        decode_delta8([0, 4 - cut], stream[:4 - cut])
    with pytest.raises(ValueError):  # the first request's range ends inside it
        decode_delta8([0, 4 - cut, 5], stream)


def test_encoder_refuses_wide_ids():
    with pytest.raises(ValueError):
        encode_delta8([0, 1], [65536])
