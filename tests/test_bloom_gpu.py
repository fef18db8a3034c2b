"""The bloom filter on the device (okv_bloom_*, objectkv_amd.bloom.DeviceBloom):
Add over rows in both kernel forms, the batched Test, WriteTo and the encode
hand-over, byte for byte against oracle/bloom_ref.py and key by key against
the host probe (okv_meta_bloom_test).  The form an add took is read from
okv_bloom_last_path."""
from __future__ import annotations

import ctypes as C
import functools
import random
import struct

import numpy as np
import pytest
import torch

import objectkv_amd as okv
from objectkv_amd import _lib
from objectkv_amd import reader as R
from objectkv_amd.bloom import DeviceBloom, pack_keys
from oracle import bloom_ref as B
from oracle import coracle as CO
from tests.test_bloom import _meta_handle, _meta_with_bloom

pytestmark = pytest.mark.gpu

LDS, GLOBAL = _lib.BLOOM_PATH_LDS, _lib.BLOOM_PATH_GLOBAL
FORMS = [pytest.param(_lib.BLOOM_FORCE_LDS, LDS, id="lds"),
         pytest.param(_lib.BLOOM_FORCE_GLOBAL, GLOBAL, id="global")]
DEFAULT = (2875518, 20)  # bloom.NewWithEstimates(100_000, 1e-6)


@pytest.fixture(scope="module")
def enc():
    e = okv.Encoder(0)
    yield e
    e.close()


def _rand_keys(seed, n, lo=1, hi=300):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(rng.integers(lo, hi + 1)), np.uint8).tobytes()
            for _ in range(n)]


def _ref(m, k, keys, start: bytes | None = None) -> bytes:
    f = B.BloomFilter.from_bytes(start) if start else B.BloomFilter(m, k)
    for key in keys:
        f.add(key)
    return f.to_bytes()


def _dev(r):
    """The key arrays of a pack_rows() / pack_keys() dict as device tensors."""
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}
    t = {k: torch.from_numpy(r[k].view(signed.get(r[k].dtype, r[k].dtype)).copy()).cuda()
         for k in ("key_arena", "key_off", "key_len")}
    torch.cuda.synchronize()  # (torch's stream is not the context's)
    return t


def _zeros(n):
    t = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the fill must not run behind a kernel on the context's stream
    return t


def _code(fn, *a, **kw):
    with pytest.raises(okv.OkvError) as e:
        fn(*a, **kw)
    return e.value.code


# ---- 1. reference add, both forced forms ------------------------------------------


@functools.lru_cache(maxsize=None)
def _reference_rows():
    keys = _rand_keys(1, 3001 - 15 - 50)
    rng = np.random.default_rng(2)
    keys += [rng.integers(0, 256, n, np.uint8).tobytes()
             for n in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 255, 256, 65535)]
    keys[1500:1500] = [b"the same key, fifty times"] * 50  # adjacent rows, colliding lanes
    assert len(keys) == 3001
    return keys, _ref(*DEFAULT, keys)


@pytest.mark.parametrize("form,path", FORMS)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_reference_add(enc, form, path, device):
    """3 001 rows into the default filter: keys of 1-300 bytes packed back to back
    (unaligned offsets), every length around the 8- and 16-byte steps, a 65 535
    byte key and 50 adjacent copies of one key."""
    keys, want = _reference_rows()
    r = pack_keys(keys)
    assert r["key_off"][1] % 8 != 0
    f = DeviceBloom(enc, *DEFAULT)
    f.add_rows(_dev(r) if device else r, form=form)
    assert f.last_path() == path
    assert f.to_bytes() == want
    f.close()


# ---- 2. length sweep ----------------------------------------------------------------


@pytest.mark.parametrize("form,path", FORMS)
def test_length_sweep(enc, form, path):
    """One key of every length 0..80 (the empty key included) into (1000, 7)."""
    rng = np.random.default_rng(3)
    keys = [rng.integers(0, 256, n, np.uint8).tobytes() for n in range(81)]
    f = DeviceBloom(enc, 1000, 7)
    f.add_rows(keys, form=form)
    assert f.last_path() == path
    assert f.to_bytes() == _ref(1000, 7, keys)
    f.close()


# ---- 3. filter shapes -----------------------------------------------------------------

SHAPES = [(1, 1), (2, 3), (63, 2), (64, 3), (65, 4), (1000, 7), (4097, 5), (2**20, 20),
          (2**20 + 1, 20), (3 * 2**20 - 7, 33)]


@pytest.mark.parametrize("form,path", FORMS)
@pytest.mark.parametrize("m,k", SHAPES)
def test_filter_shapes(enc, m, k, form, path):
    """257 rows: the last partial word, the edges of the 2^20-bit LDS slices (one,
    two and three slices) and the location index pattern past its period of 4."""
    keys = _rand_keys(4, 257, 1, 40)
    f = DeviceBloom(enc, m, k)
    assert f.info() == (m, k, m, 24 + 8 * ((m + 63) // 64))
    f.add_rows(_dev(pack_keys(keys)), form=form)
    assert f.last_path() == path
    assert f.to_bytes() == _ref(m, k, keys)
    f.close()


# ---- 4. row counts, automatic form ------------------------------------------------------


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_row_counts(enc, n):
    keys = _rand_keys(5, 1025, 1, 24)[:n]
    f = DeviceBloom(enc, *DEFAULT)
    f.add_rows(pack_keys(keys))
    assert f.last_path() in ((LDS, GLOBAL) if n else (0,))
    got = f.to_bytes()
    assert got == _ref(*DEFAULT, keys)
    if n == 0:
        assert not any(got[24:])
    f.close()


def test_automatic_form_at_its_threshold(enc):
    """The rule of DESIGN.md 19.3: a filter of up to 1 MiB takes the LDS form from
    2^19 locations (rows x k) on, the global form below."""
    keys = _rand_keys(12, 26215, 1, 12)
    assert 26214 * 20 < 2**19 <= 26215 * 20
    ref = B.BloomFilter(*DEFAULT)
    for key in keys[:-1]:
        ref.add(key)
    f = DeviceBloom(enc, *DEFAULT).add_rows(keys[:-1])
    assert f.last_path() == GLOBAL and f.to_bytes() == ref.to_bytes()
    ref.add(keys[-1])
    f.clear().add_rows(keys)
    assert f.last_path() == LDS and f.to_bytes() == ref.to_bytes()
    f.close()


# ---- 5. accumulation ------------------------------------------------------------------------


def test_accumulation_read_from_clear_and_async(enc):
    a, b = _rand_keys(6, 400), _rand_keys(7, 300)
    both = _ref(*DEFAULT, a + b)
    f = DeviceBloom(enc, *DEFAULT)
    f.add_rows(a, form=_lib.BLOOM_FORCE_LDS).add_rows(b, form=_lib.BLOOM_FORCE_GLOBAL)
    assert f.to_bytes() == both
    # starting from ReadFrom of a pre-populated filter
    g = DeviceBloom.from_bytes(enc, _ref(*DEFAULT, a) + b"trailing bytes are ignored")
    assert g.info() == f.info()
    g.add_rows(b)
    assert g.to_bytes() == both
    g.clear()
    assert g.to_bytes() == B.BloomFilter(*DEFAULT).to_bytes()
    # add + WriteTo only enqueued, one synchronisation
    dst = _zeros(g.write_to_bytes)
    g.add_rows(_dev(pack_keys(a)), sync=False)
    g.add_rows(_dev(pack_keys(b)), sync=False)
    g.write_to_device(dst, sync=False)
    enc.sync()
    assert dst.cpu().numpy().tobytes() == both
    f.close()
    g.close()


# ---- 6. reduction past 32 bits ------------------------------------------------------------------


@pytest.mark.parametrize("m", [2**32 - 5, 2**32 + 11])
def test_reduction_past_32_bits(enc, m):
    """k = 20, 300 keys: the filter (512 MiB of words) takes the global form; the
    non-zero bytes of WriteTo are exactly those BloomFilter._locations gives."""
    keys = _rand_keys(8, 300, 1, 40)
    ref = B.BloomFilter.__new__(B.BloomFilter)  # m and k only: no 67 M-entry word list
    ref.m, ref.k = m, 20
    want = {i: v for i, v in enumerate(struct.pack(">QQQ", m, 20, m)) if v}
    for key in keys:
        for loc in ref._locations(key):
            at = 24 + 8 * (loc >> 6) + 7 - ((loc & 63) >> 3)
            want[at] = want.get(at, 0) | (1 << (loc & 7))
    f = DeviceBloom(enc, m, 20)
    r = _dev(pack_keys(keys))
    assert _code(f.add_rows, r, form=_lib.BLOOM_FORCE_LDS) == _lib.OKV_E_ARG
    f.add_rows(r)
    assert f.last_path() == GLOBAL
    dst = _zeros(f.write_to_bytes)
    f.write_to_device(dst)
    at = torch.nonzero(dst).flatten()
    got = dict(zip(at.cpu().tolist(), dst[at].cpu().tolist()))
    assert got == want
    del dst
    f.close()


# ---- 7. probe ---------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _probe_case():
    members = [b"key%06d" % i for i in range(0, 10000, 2)]
    f = B.default_filter()
    for k in members:
        f.add(k)
    probes = members + [b"key%06d" % i for i in range(1, 10000, 2)] + [b""] + \
        _rand_keys(9, 20000 - 10001)
    return members, f, probes, [int(f.test(k)) for k in probes]


def test_probe_matches_reference_and_host_probe(enc):
    members, ref, probes, want = _probe_case()
    assert len(probes) == 20000
    f = DeviceBloom(enc, *DEFAULT).add_rows(members)
    assert f.to_bytes() == ref.to_bytes()
    got = f.test_rows(probes)
    assert got.tolist() == want
    assert got[:len(members)].all()
    # device rows, device result
    out = _zeros(len(probes))
    f.test_rows(_dev(pack_keys(probes)), out=out)
    assert out.cpu().numpy().tolist() == want
    # the host probe on the parsed meta block
    rc, h = _meta_handle(_meta_with_bloom(f.to_bytes()))
    assert rc == 0
    try:
        for i in random.Random(10).sample(range(len(probes)), 500):
            assert _lib.lib().okv_meta_bloom_test(h, probes[i], len(probes[i])) == got[i]
    finally:
        _lib.lib().okv_meta_free(h)
    f.close()


@pytest.mark.parametrize("m,k,length,nwords", [
    (64, 3, 64, 1), (1000, 7, 1000, 16), (10, 2, 0, 0), (100, 0, 100, 2), (129, 4, 200, 4)])
def test_probe_small_filters(enc, m, k, length, nwords):
    """The hand-built filters of tests/test_bloom.py through read_from: a bitset
    length that differs from m, k = 0, an empty bitset."""
    rng = np.random.default_rng(m * 31 + k)
    words = [int(x) for x in rng.integers(0, 2**63, nwords, dtype=np.uint64)]
    bb = struct.pack(f">QQQ{nwords}Q", m, k, length, *words)
    ref = B.BloomFilter.from_bytes(bb)
    f = DeviceBloom.from_bytes(enc, bb)
    assert f.info() == (m, k, length, len(bb)) and f.to_bytes() == bb
    keys = [b"p%d" % i for i in range(500)]
    assert f.test_rows(keys).tolist() == [int(ref.test(key)) for key in keys]
    if length != m:  # Go's bitset.Set would grow the set
        assert _code(f.add_rows, keys) == _lib.OKV_E_ARG
        assert f.to_bytes() == bb
    f.close()


def test_probe_zero_m_and_read_from_errors(enc):
    f = DeviceBloom.from_bytes(enc, struct.pack(">QQQQ", 0, 3, 64, 1))
    assert _code(f.test_rows, [b"x"]) == _lib.OKV_E_ARG  # Go: integer divide by zero
    f.close()
    for bb in (b"", b"\x00" * 23, struct.pack(">QQQ", 64, 3, 65),
               struct.pack(">QQQQ", 640, 3, 640, 1), struct.pack(">QQQ", 64, 3, 2**64 - 1)):
        assert _code(DeviceBloom.from_bytes, enc, bb) == _lib.OKV_E_ARG


# ---- 8. encode hand-over ----------------------------------------------------------------------------------


def _sorted_rows(first_len, last_len):
    rng = random.Random(11)
    mid = {b"k" + bytes(rng.randrange(256) for _ in range(rng.randrange(9, 40))) for _ in range(2998)}
    while len(mid) < 2998:
        mid.add(b"k" + bytes(rng.randrange(256) for _ in range(40)))
    rows = [(b"a" * first_len, b"first")] + \
        [(k, bytes(rng.randrange(256) for _ in range(rng.randrange(0, 300)))) for k in sorted(mid)] + \
        [(b"z" * last_len, b"last")]
    assert len(rows) == 3000 and rows == sorted(rows)
    return rows


@pytest.mark.parametrize("first_len,last_len,aligned", [(2, 9, True), (2, 8, False)])
def test_encode_hand_over(enc, decoder, first_len, last_len, aligned):
    """Encoder.encode / encode_device / GpuSegmentWriter with a DeviceBloom: the
    rows are added on the device and the filter bytes reach the meta block device
    to device, at an 8-aligned and at an odd offset; the file is the oracle
    writer's with bloom_ref's bytes, trailer included."""
    rows = _sorted_rows(first_len, last_len)
    keys = [k for k, _ in rows]
    bb = _ref(*DEFAULT, keys)
    w = CO.Writer()
    for k, v in rows:
        assert w.write_row(k, v) == 0
    w.set_bloom(bb)
    rc, want, want_meta = w.close()
    assert rc == 0
    at = len(want) - 25 - len(want_meta) + 13 + first_len + last_len  # of the filter bytes
    assert want[at:at + len(bb)] == bb
    assert (at % 8 == 0) if aligned else (at % 2 == 1)
    # host buffers
    f = DeviceBloom(enc, *DEFAULT)
    got = enc.encode(rows, bloom=f)
    assert f.last_path() in (LDS, GLOBAL)
    assert got.seg.tobytes() == want and got.meta() == want_meta
    f.close()
    # device tensors
    r = okv.pack_rows(rows)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16,
              np.dtype(np.uint32): np.int32}
    t = {k: torch.from_numpy(v.view(signed.get(v.dtype, v.dtype)).copy()).cuda()
         for k, v in r.items()}
    seg_t = _zeros(len(want) + 4096)
    f = DeviceBloom(enc, *DEFAULT)
    eo = enc.encode_device(t, len(rows), {"seg": seg_t}, bloom=f,
                           key_arena_bytes=r["key_arena"].size,
                           val_arena_bytes=r["val_arena"].size)
    assert eo.file_bytes == len(want)
    assert seg_t[:eo.file_bytes].cpu().numpy().tobytes() == want
    assert f.to_bytes() == bb
    f.close()
    # the writer mirror: no per-row add, the same file
    f = DeviceBloom(enc, *DEFAULT)
    gw = okv.GpuSegmentWriter(enc, bloom=f)
    for k, v in rows:
        gw.WriteRow(k, v)
    flen, meta = gw.Close()
    assert flen == len(want) and meta == want_meta and gw.data().tobytes() == want
    f.close()
    # the segment reads back: metadata parses, the host probe and GetRow find every member
    rc, h = _meta_handle(want_meta)
    assert rc == 0 and _lib.lib().okv_meta_has_bloom(h) == 1
    try:
        assert all(_lib.lib().okv_meta_bloom_test(h, k, len(k)) == 1 for k in keys)
    finally:
        _lib.lib().okv_meta_free(h)
    pr = R.SegmentReader(want, len(want), decoder)
    for k, v in rows[::97] + [rows[-1]]:
        assert pr.GetRow(k).Value == (v or None)


# ---- 9. arguments ---------------------------------------------------------------------------------------------


def test_arguments(enc):
    L = _lib.lib()
    r = pack_keys([b"a", b"bc"])
    rows = _lib.Rows(r["key_arena"].ctypes.data, r["key_off"].ctypes.data,
                     r["key_len"].ctypes.data, None, None, None, 2, int(r["key_arena"].size), 0)
    out = np.zeros(2, np.uint8)
    assert L.okv_bloom_add_rows(enc._ctx, None, C.byref(rows), 0) == _lib.OKV_E_ARG
    assert L.okv_bloom_test_rows(enc._ctx, None, C.byref(rows), out.ctypes.data, 0) == _lib.OKV_E_ARG
    assert L.okv_bloom_write_to(enc._ctx, None, out.ctypes.data, 2, 0) == _lib.OKV_E_ARG
    assert L.okv_bloom_info(None, None, None, None, None) == _lib.OKV_E_ARG
    assert L.okv_bloom_last_path(None) == 0
    f = DeviceBloom(enc, 1000, 7)
    assert L.okv_bloom_add_rows(None, f._h, C.byref(rows), 0) == _lib.OKV_E_ARG
    assert L.okv_bloom_add_rows(enc._ctx, f._h, None, 0) == _lib.OKV_E_ARG
    both = _lib.BLOOM_FORCE_LDS | _lib.BLOOM_FORCE_GLOBAL
    assert L.okv_bloom_add_rows(enc._ctx, f._h, C.byref(rows), both) == _lib.OKV_E_ARG
    other = okv.Encoder(0)  # a filter belongs to the context that created it
    try:
        assert L.okv_bloom_add_rows(other._ctx, f._h, C.byref(rows), 0) == _lib.OKV_E_ARG
        assert L.okv_bloom_clear(other._ctx, f._h) == _lib.OKV_E_ARG
        assert _code(other.encode, [(b"a", b"v")], bloom=f) == _lib.OKV_E_ARG
    finally:
        other.close()
    assert f.to_bytes() == B.BloomFilter(1000, 7).to_bytes()  # nothing was added
    # WriteTo: capacity and the device destination's alignment
    need = f.write_to_bytes
    host = np.zeros(need, np.uint8)
    assert L.okv_bloom_write_to(enc._ctx, f._h, host.ctypes.data, need - 1, 0) == _lib.OKV_E_CAPACITY
    dst = _zeros(need + 8)
    assert _code(f.write_to_device, dst[:need - 1]) == _lib.OKV_E_CAPACITY
    assert dst[1:].data_ptr() % 2 == 1
    assert _code(f.write_to_device, dst[1:]) == _lib.OKV_E_ARG
    assert not dst.any()
    f.close()
    # k beyond the device paths' cap (Go has none)
    g = DeviceBloom(enc, 1000, 4097)
    assert g.info()[1] == 4097
    assert _code(g.add_rows, [b"a"]) == _lib.OKV_E_ARG
    assert _code(g.test_rows, [b"a"]) == _lib.OKV_E_ARG
    g.close()
