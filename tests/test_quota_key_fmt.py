"""istio_amd/csrc/quota_key_fmt.h -- the bytes memquota's makeKey writes for int64, float64 and bool
dimension values -- compiled for the host as a stand-alone program (tests/quota_key_host.cpp) with
AddressSanitizer and UBSan, every value formatted into a heap buffer of exactly the counted length,
against tests/quota_keys_model.py (pinned by test_quota_keys_model.py) on 20k seeded values."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import quota_keys_model as Q  # noqa: E402

INT64, DOUBLE, BOOL = 2, 3, 4
M64 = (1 << 64) - 1


def values(seed=17, n=20000):
    """[(kind, 64 bits)]: every int64 +-2^k, +-(2^k - 1); doubles as random bit patterns, every
    special, subnormals, powers of two and their neighbours; both bools; then seeded ones."""
    out = [(BOOL, 0), (BOOL, 1)]
    for k in range(64):
        for v in (1 << k, -(1 << k), (1 << k) - 1, -((1 << k) - 1)):
            if -(1 << 63) <= v < (1 << 63):
                out.append((INT64, v & M64))
    specials = [0x0, 1 << 63, 0x7FF0 << 48, 0xFFF0 << 48, 0x7FF8 << 48, (0xFFF0 << 48) | 1, (0x7FF0 << 48) | 1,
                0x3FF0 << 48, 1, (1 << 63) | 1, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF]
    out += [(DOUBLE, b) for b in specials]
    for e in range(0, 0x7FF, 7):
        out += [(DOUBLE, e << 52), (DOUBLE, (e << 52) | ((1 << 52) - 1)), (DOUBLE, (1 << 63) | (e << 52) | 1)]
    rng = np.random.default_rng(seed)
    out += [(DOUBLE, int(b)) for b in rng.integers(0, 1 << 64, 6000, dtype=np.uint64)]
    out += [(DOUBLE, int(b)) for b in rng.integers(0, 1 << 52, 1500, dtype=np.uint64)]  # subnormals
    out += [(DOUBLE, struct.unpack("<Q", struct.pack("<d", float(x)))[0]) for x in rng.normal(0, 1e3, 1500)]
    out += [(DOUBLE, struct.unpack("<Q", struct.pack("<d", float(x)))[0]) for x in rng.integers(-1000, 1000, 500)]
    rest = n - len(out)
    out += [(INT64, int(b)) for b in rng.integers(0, 1 << 64, rest // 2, dtype=np.uint64)]
    shifts = rng.integers(0, 64, rest - rest // 2)
    out += [(INT64, (int(b) >> int(s)) & M64) for b, s in
            zip(rng.integers(0, 1 << 64, rest - rest // 2, dtype=np.uint64), shifts)]
    return out


def model(kind, bits):
    if kind == BOOL:
        return Q.value_bytes(bool(bits))
    if kind == INT64:
        return Q.value_bytes(bits - (1 << 64) if bits >> 63 else bits)
    return Q.PAD + Q.format_bits_b(bits)


def build_host_program(outdir) -> str:
    """tests/quota_key_host.cpp with the host compiler, ASan + UBSan, the runtimes linked statically
    (as tests/test_rfc3339_independent.py builds its program, and for its reason)."""
    exe = os.path.join(str(outdir), "quota_key_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "istio_amd", "csrc"), os.path.join(HERE, "quota_key_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "building the sanitized host program failed (it needs g++ with its static " \
                              "libasan / libubsan):\n" + r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("quota_key_host"))


def test_formatter_agrees_with_model_under_sanitizers(host_exe):
    vals = values()
    assert len(vals) >= 20000
    text = "".join("%d %016x\n" % v for v in vals)
    r = subprocess.run([host_exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(vals)
    bad = [(k, hex(b), bytes.fromhex(ln), model(k, b)) for (k, b), ln in zip(vals, lines) if bytes.fromhex(ln) != model(k, b)]
    assert not bad, bad[:6]
    want = [model(k, b) for k, b in vals]
    assert all(w.startswith(Q.PAD) and len(w) > 32 for w in want)
    tails = {w[32:] for w in want}
    assert {b"true", b"false", b"+Inf", b"-Inf", b"NaN", b"0p-1074", b"-0p-1074", b"1p-1074", b"-8000000000000000",
            b"7fffffffffffffff", b"0", b"-1", b"4503599627370496p-52"} <= tails
    assert sum(b"p+" in t for t in tails) > 1000 and sum(b"p-" in t for t in tails) > 1000
