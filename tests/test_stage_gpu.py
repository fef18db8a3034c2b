"""Host mode against device mode for the six batched entry points that stage an okv_rows
(okv_stage.hpp): the same input through both, every output array and
total compared, at the key counts where the staged columns cross a 256-byte line; and
three inputs the staging offsets could get wrong."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest
import torch

import objectkv_amd as okv
from objectkv_amd import _lib, get as G, range as RG, snap as S
from objectkv_amd.bloom import key_rows, pack_keys
from objectkv_amd.sst import _ptr
from oracle import bloom_ref as B
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu

NS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
ASC, DESC = P.DirectionAscending, P.DirectionDescending
SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32,
          np.dtype(np.uint16): np.int16}
TORCH = {np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32,
         np.dtype(np.uint64): torch.int64, np.dtype(np.uint16): torch.int16}
# rows of segment 1 with an empty value that segment 2 does not hide
NIL = tuple(i for i in range(14, 600, 28) if i % 10)


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.copy().view(SIGNED.get(a.dtype, a.dtype))).cuda()


def _write(rows):
    w = P.SegmentWriter(P.SegmentWriterOptions(BloomFilter=B.BloomFilter(8192, 3)))
    for k, v in rows:
        w.WriteRow(k, v)
    n, meta = w.Close()
    return bytes(w.external), n, meta


class World:
    """Segment 1 (level 1): 300 rows k0000, k0002, ... in 4 KiB blocks.  Segment 2 (level 0,
    newer): every tenth key again, every twentieth as a tombstone."""

    def __init__(self, decoder):
        rng = random.Random(11)
        old = [(b"k%04d" % i, b"" if i in NIL else
                bytes(rng.getrandbits(8) for _ in range(rng.choice((1, 15, 16, 17, 40, 200)))))
               for i in range(0, 600, 2)]
        new = [(b"k%04d" % i, b"" if i % 20 == 0 else b"new%d" % i) for i in range(0, 600, 10)]
        self.dec, self.segs, tuples = decoder, [], []
        for sid, lvl, rows in ((1, 1, old), (2, 0, new)):
            data, _n, meta = _write(rows)
            pmd, md = P.bytes_to_metadata(meta), okv.bytes_to_metadata(meta)
            t = _dev(np.frombuffer(data + bytes(RG.ARENA_SPARE), np.uint8))
            ix = okv.DeviceIndex.from_metadata(decoder, md)
            bl = okv.DeviceBloom.from_bytes(decoder, pmd.BloomFilter)
            rr = RG.ResidentRows(decoder, t, len(data), md)
            assert not rr.status.any() and rr.n == len(rows)
            self.segs.append(dict(t=t, bytes=len(data), ix=ix, bl=bl, md=md, rows=rr))
            tuples.append((t, len(data), ix, bl, md.compression, lvl, sid, pmd.FirstKey,
                           pmd.LastKey))
        assert self.segs[0]["ix"].info()[0] > 1  # more than one block
        self.snap = okv.DeviceSnapshot(decoder, tuples)

    def close(self):
        self.snap.close()
        for s in self.segs:
            s["ix"].close()
            s["bl"].close()


@pytest.fixture(scope="module")
def world(decoder):
    w = World(decoder)
    yield w
    w.close()


def _keys(n):
    """Hits (even numbers), misses (odd numbers, and a suffix no row has) and, from the
    21st key on, keys whose newest row is a tombstone."""
    return [(b"k%04d" if i % 4 != 3 else b"k%04dx") % (i * 7 % 600) for i in range(n)]


def _both(keys):
    """-> (host key arrays, device key tensors, n, key_arena_bytes)"""
    pk = keys if isinstance(keys, dict) else pack_keys(keys)
    # (the device arrays carry 16 spare elements; a NULL host arena is 16 device bytes)
    dk = {k: _dev(np.concatenate([np.zeros(0, np.uint8) if v is None else v,
                                  np.zeros(16, np.uint8 if v is None else v.dtype)]))
          for k, v in pk.items()}
    kab = 0 if pk["key_arena"] is None else int(pk["key_arena"].size)
    return pk, dk, int(pk["key_len"].size), kab


def _out(cols, n, arena):
    out = {k: torch.full((n,), -3, dtype=TORCH[np.dtype(t)], device="cuda") for k, t in cols}
    out["val_arena"] = torch.full((arena,), 0xEE, dtype=torch.uint8, device="cuda")
    return out


def _same(host, dev, cols, totals):
    for name, t in cols:
        got = getattr(dev, name).cpu().numpy().view(t)
        assert np.array_equal(got, getattr(host, name)), name
    for name in totals:
        assert getattr(dev, name) == getattr(host, name), name
    nb = host.val_bytes
    assert dev.val_arena.cpu().numpy()[:nb].tobytes() == host.val_arena[:nb].tobytes()


GET_TOTALS = ("n_found", "n_fallback", "val_bytes", "blocks_searched")


def _get(w, keys, **kw):
    s = w.segs[0]
    return G.get_rows(w.dec, s["t"], s["bytes"], s["ix"], keys, bloom=s["bl"],
                      compression=s["md"].compression, **kw)


def _parity(w, keys):
    """All six entry points over `keys`, host mode against device mode -> the host results."""
    dec = w.dec
    pk, dk, n, kab = _both(keys)
    torch.cuda.synchronize()  # (the decoder has its own stream)
    kw = dict(n_rows=n, key_arena_bytes=kab)

    # okv_bloom_test_rows, okv_bloom_add_rows (the words read back by okv_bloom_write_to)
    bl = w.segs[0]["bl"]
    maybe = bl.test_rows(pk)
    d_maybe = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bl.test_rows(dk, out=d_maybe, **kw)
    assert np.array_equal(d_maybe.cpu().numpy(), maybe)
    words = []
    for rows, more in ((pk, {}), (dk, kw)):
        f = okv.DeviceBloom(dec, 1000, 3)
        words.append(f.add_rows(rows, **more).to_bytes())
        f.close()
    assert words[0] == words[1] and len(words[0]) > 24

    # okv_get_rows, okv_snap_get_rows
    g = _get(w, pk)
    out = _out(G._OUT, n, g.val_bytes + 64)
    torch.cuda.synchronize()
    _same(g, _get(w, dk, out=out, **kw), G._OUT, GET_TOTALS)
    r = S.snap_get_rows(dec, w.snap, pk)
    out = _out(S._OUT, n, r.val_bytes + 64)
    torch.cuda.synchronize()
    _same(r, S.snap_get_rows(dec, w.snap, dk, out=out, **kw), S._OUT, S._TOTALS)

    # okv_seek_rows: key i into segment i % 2, ascending and descending by turns
    srcs = [s["rows"] for s in w.segs]
    src_of = np.arange(n, dtype=np.uint32) % 2
    dirs = np.where(np.arange(n) // 2 % 2 == 0, ASC, DESC).astype(np.uint8)
    lo, hi = RG.seek_rows(dec, srcs, pk, src_of, dirs)
    so = {"row_lo": _dev(np.full(n, -1, np.int64)), "row_hi": _dev(np.full(n, -1, np.int64))}
    d_src, d_dir = _dev(src_of), _dev(dirs)
    torch.cuda.synchronize()
    RG.seek_rows(dec, srcs, dk, d_src, d_dir, out=so, **kw)
    assert np.array_equal(so["row_lo"].cpu().numpy().view(np.uint64), lo)
    assert np.array_equal(so["row_hi"].cpu().numpy().view(np.uint64), hi)

    # okv_gather_rows: row 11 i of segment i % 2 (it takes no okv_rows: n picked rows)
    row = np.array([i * 11 % srcs[i % 2].n for i in range(n)], np.uint64)
    d_row = _dev(row)
    torch.cuda.synchronize()
    gh = RG.gather_rows(dec, srcs, d_src, d_row, n)
    go = {k: torch.full((n,), -3, dtype=TORCH[np.dtype(t)], device="cuda") for k, t in RG._GATHER}
    go["key_arena"] = torch.zeros(gh.key_bytes + 16, dtype=torch.uint8, device="cuda")
    go["val_arena"] = torch.zeros(gh.val_bytes + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gd = RG.gather_rows(dec, srcs, d_src, d_row, n, out=go)
    for name, t in RG._GATHER:
        assert np.array_equal(getattr(gd, name).cpu().numpy().view(t), getattr(gh, name)), name
    assert (gd.key_bytes, gd.val_bytes) == (gh.key_bytes, gh.val_bytes)
    for name, nb in (("key_arena", gh.key_bytes), ("val_arena", gh.val_bytes)):
        assert getattr(gd, name).cpu().numpy()[:nb].tobytes() == \
            getattr(gh, name)[:nb].tobytes(), name
    return dict(maybe=maybe, get=g, snap=r, lo=lo, hi=hi, gather=gh)


@pytest.mark.parametrize("n", NS)
def test_host_mode_is_device_mode(world, n):
    h = _parity(world, _keys(n))
    assert len(h["get"].state) == n and h["gather"].key_bytes > 0
    if n >= 31:  # the mix: hits, misses and an L0 tombstone; values of several blocks
        states = set(h["get"].state.tolist())
        assert _lib.GET_FOUND in states
        assert states & {_lib.GET_BLOOM_NEGATIVE, _lib.GET_NOT_IN_BLOCK}
        assert {_lib.SNAP_FOUND, _lib.SNAP_NO_ROWS, _lib.SNAP_DELETED} <= \
            set(h["snap"].state.tolist())
        assert 0 < h["get"].n_found < n and h["get"].val_bytes > 0
        assert h["get"].blocks_searched > 1 and (h["hi"] > h["lo"]).any()
        i = h["get"].state.tolist().index(_lib.GET_FOUND)
        assert h["get"].value(i) is not None


def test_every_key_empty_and_no_arena(world):
    """key_arena_bytes == 0 with a NULL arena: the offsets and lengths start the buffer."""
    n = 33
    keys = {"key_arena": None, "key_off": np.zeros(n, np.uint64), "key_len": np.zeros(n, np.uint16)}
    h = _parity(world, keys)
    assert h["get"].n_found == 0 and h["snap"].n_found == 0 and h["get"].val_bytes == 0


def test_host_mode_without_val_pos(world):
    """val_pos NULL in host mode: the column keeps its room on the device, nothing is
    copied back for it, and every other output and the values are as with it."""
    w, n = world, 65
    keys = _keys(n)
    R, dev, _keep = key_rows(keys, None, None)
    assert not dev
    s = w.segs[0]
    for cols, make, call, want in (
            (G._OUT, lambda p, a, cap: _lib.GetOut(*p, a, cap, 0, 0, 0, 0),
             lambda o: _lib.lib().okv_get_rows(w.dec._ctx, _ptr(s["t"]), s["bytes"], s["ix"]._h,
                                               s["bl"]._h, C.byref(R), s["md"].compression,
                                               C.byref(o), 0),
             _get(w, keys)),
            (S._OUT, lambda p, a, cap: _lib.SnapOut(*p, a, cap, 0, 0, 0, 0, 0, 0),
             lambda o: _lib.lib().okv_snap_get_rows(w.dec._ctx, w.snap._h, C.byref(R),
                                                    C.byref(o), 0),
             S.snap_get_rows(w.dec, w.snap, keys))):
        assert want.val_bytes > 0
        arrays = {k: np.full(n, 0x55, t) for k, t in cols if k != "val_pos"}
        arena = np.zeros(want.val_bytes, np.uint8)
        o = make([_ptr(arrays.get(k)) for k, _ in cols], _ptr(arena), arena.size)
        assert call(o) == 0, w.dec.error()
        for k in arrays:
            assert np.array_equal(arrays[k], getattr(want, k)), k
        assert (o.n_found, o.val_bytes) == (want.n_found, want.val_bytes)
        assert arena.tobytes() == want.val_arena[:want.val_bytes].tobytes()


def test_every_found_value_nil(world):
    """val_bytes == 0 with an arena given: the call returns before it reserves a device
    arena; every key is found with Go's nil."""
    keys = [b"k%04d" % i for i in NIL]
    n = len(keys)
    h = _parity(world, keys)
    for res, found in ((_get(world, keys, val_cap=64), _lib.GET_FOUND),
                       (S.snap_get_rows(world.dec, world.snap, keys, val_cap=64), _lib.SNAP_FOUND)):
        assert res.state.tolist() == [found] * n and res.n_found == n
        assert res.val_bytes == 0 and not res.val_len.any() and not res.val_arena.any()
        assert [res.value(i) for i in range(n)] == [None] * n
    assert h["get"].val_bytes == 0 and h["snap"].val_bytes == 0
