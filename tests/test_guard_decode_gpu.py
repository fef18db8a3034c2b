"""Caller buffers of okv_decode_blocks (OKV_F_DEVICE_PTRS): every input and
output is a tests/guarded.py frame -- poisoned, with guard bands inside the
same allocation, at base 0 and base 16 of a 128-byte line -- and each case
asserts, per route of the dispatcher,

  G  the guards of every frame are intact after every call, errors included;
  X  inside the extents okv_sst.h defines (n_rows rows, key_bytes / val_bytes
     of the arenas with their zero padding, nblk / nblk + 1 per-block entries)
     every output equals oracle.coracle.decode_soa bit for bit -- under both
     poisons, so a byte the kernels forgot to write cannot pass;
  N  outputs of a call refused with OKV_E_ARG are untouched;
  D  the result does not depend on the bytes around the segment (they are
     poison here, zeros everywhere else in the suite).

Outputs are sized exactly by okv_decode_plan, so the 16-byte padding of the
last region ends exactly at key_cap / val_cap."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import objectkv_amd as okv
from objectkv_amd import _lib
from oracle import coracle as CO
from tests import guarded as G
from tests.conftest import descs_of, unpack
from tests.test_decode_gpu import _mixed_segment
from tests.test_tile_gpu import TILE, _fill_to, _segment

pytestmark = pytest.mark.gpu

POISONS = [0xA5, 0x5A]
BASES = [0, 16]
ROW_ARRAYS = (("key_off", np.uint64), ("key_len", np.uint16), ("val_off", np.uint64),
              ("val_len", np.uint32))
NONE, ZSTD = _lib.COMP_NONE, _lib.COMP_ZSTD


def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def nofused():
    dec = okv.Decoder(0, flags=_lib.OPEN_NO_FUSED)
    yield dec
    dec.close()


@pytest.fixture(scope="module")
def onepass():
    dec = okv.Decoder(0, flags=_lib.OPEN_ZSTD_ONE_PASS)
    yield dec
    dec.close()


# ---- segments (built once) and their oracle results ---------------------------

_SEGS, _REFS = {}, {}


def _edges_segment():
    """Six large blocks at the tile pass's edges: records across and around a
    16 KiB tile edge (test_tile_gpu._boundary_segment), values across and just
    past one followed by a long key (_line_cut_segment), a block ending exactly
    on a tile edge; the last block ends at the segment's last byte, with
    seg_bytes, its key bytes and its value bytes all not multiples of 16."""
    rng = np.random.default_rng(41)
    blocks = [
        _fill_to(TILE + 3 - (6 + 20 + 1000), 12, rng) + [(20, 1000)] + [(33, 777)] * 3,
        _fill_to(2 * TILE - 6 - (6 + 20 + 1000), 12, rng) + [(20, 1000)] + [(33, 777)] * 3,
        _fill_to(TILE - 1500 - (6 + 16), 16, rng) + [(16, 3000), (16, 40)],
        _fill_to(2 * TILE + 9 - (6 + 16 + 600), 16, rng) + [(16, 600), (330, 300), (30, 0), (30, 7)],
        _fill_to(2 * TILE, 16, rng),
    ]
    last = _fill_to(TILE + 5000, 13, rng)
    for tail in ((7, 3), (5, 1), (9, 2), (3, 5), (11, 6)):
        cand = last + [tail]
        ks, vs = sum(k for k, _ in cand), sum(v for _, v in cand)
        total = 5 * 65536 + sum(6 + k + v for k, v in cand)
        if ks % 16 and vs % 16 and total % 16:
            break
    else:
        raise AssertionError("no tail gives odd extents")
    blocks.append(cand)
    seg, d = _segment(blocks, 42)
    d = d.copy()
    end = int(d[-1, 0] + d[-1, 2])
    d[-1, 1] = d[-1, 2]  # the block ends at the segment's last byte
    seg = seg[:end]
    assert len(seg) % 16 != 0 and len(seg) // 6 > 16384
    return seg, d


def _crafted(large):
    import json
    from tests.conftest import GOLDEN
    with open(GOLDEN) as f:
        case = {c["name"]: c for c in json.load(f)["cases"]}["crafted_edges"]
    seg, d = unpack(case["segment_z"]), descs_of(case)
    if large:  # the buffer padded so the blocks average over 16 KiB: the large-block pass
        seg = seg + bytes(max(0, 16385 * d.shape[0] - len(seg)) + 4096)
        seg = seg + bytes(3 if len(seg) % 16 == 0 else 0)
    return seg, d


def _zstd4():
    from oracle import pyoracle as P
    from tests import zstd_cases as ZC
    zseg, _, _ = ZC.Z.zstd_segment(ZC._rows(41, 400), 3584, 4096, level=3)
    zd = np.array([st.desc() for st in P.bytes_to_metadata(ZC._meta_of(zseg)).entries[:4]],
                  np.uint64).reshape(-1, 4)
    assert zd.shape[0] == 4
    return zseg[:int(zd[-1][0] + zd[-1][1])], zd


def _small600():
    kinds = ["s"] * 600
    kinds[300] = "M"
    return _mixed_segment(kinds, 32)


def _ragged_small(n, seed):
    """n small blocks of 3..40 rows with keys of 1..20 and values of 0..90 bytes,
    at odd offsets: no region is a multiple of 16 bytes, so every block has
    zero padding to write, the last one's ending exactly at the capacity."""
    rng = np.random.default_rng(seed)
    seg, descs = bytearray(), []
    for b in range(n):
        body = bytearray()
        while True:
            shape = [(int(rng.integers(1, 21)), int(rng.integers(0, 91)))
                     for _ in range(int(rng.integers(3, 41)))]
            if sum(k for k, _ in shape) % 16 and sum(v for _, v in shape) % 16:
                break
        for kl, vl in shape:
            body += kl.to_bytes(2, "little") + vl.to_bytes(4, "little")
            body += rng.integers(0, 256, kl + vl, dtype=np.uint8).tobytes()
        off = len(seg) + int(rng.choice([0, 1, 5, 11]))
        seg += bytes(off - len(seg)) + body + bytes(0 if b == n - 1 else int(rng.integers(0, 9)))
        descs.append((off, len(seg) - off, len(body), 0))
    if len(seg) % 16 == 0:
        seg += b"\0"
        descs[-1] = (descs[-1][0], descs[-1][1] + 1, descs[-1][2], 0)
    return bytes(seg), np.array(descs, np.uint64).reshape(-1, 4)


def _odd_tail(seg, d):
    """The same blocks with the buffer cut to the last block's last record byte
    when that makes seg_bytes % 16 != 0 (the kernels' 16-byte loads then reach
    past seg_bytes, into poison)."""
    d = d.copy()
    end = int(d[-1, 0] + d[-1, 2])
    if end % 16:
        d[-1, 1] = d[-1, 2]
        seg = seg[:end]
    return seg, d


BUILDERS = {
    "fused": lambda: _odd_tail(*_mixed_segment(["s"] * 8, 31)),
    "no_fused": lambda: _odd_tail(*_mixed_segment(["s", "s", "M", "s"] * 2, 35)),
    "small_gather": _small600,
    "ragged": lambda: _ragged_small(9, 36),
    "tile_big": lambda: _mixed_segment(["L", "M", "L", "L"], 34),
    "tile_edges": _edges_segment,
    "zstd": _zstd4,
    "crafted": lambda: _crafted(False),
    "crafted_large": lambda: _crafted(True),
}
# route -> (context fixture name, compression, okv_last_path or None)
ROUTES = {
    "fused": ("decoder", NONE, 1),
    "no_fused": ("nofused", NONE, 66),
    "small_gather": ("decoder", NONE, 66),
    "fused_ragged": ("decoder", NONE, 1),
    "no_fused_ragged": ("nofused", NONE, 66),
    "tile_big": ("decoder", NONE, 68),
    "tile_edges": ("decoder", NONE, None),
    "zstd": ("decoder", ZSTD, 129),
    "zstd_one_pass": ("onepass", ZSTD, 129),
    "crafted": ("decoder", NONE, None),
    "crafted_large": ("decoder", NONE, None),
}


def _segment_of(route):
    name = "zstd" if route.startswith("zstd") else "ragged" if route.endswith("ragged") else route
    if name not in _SEGS:
        seg, d = BUILDERS[name]()
        _SEGS[name] = (bytes(seg), np.ascontiguousarray(d, np.uint64).reshape(-1, 4))
    return name, _SEGS[name]


def _ref_of(name, comp, index_only):
    key = (name, comp, index_only)
    if key not in _REFS:
        seg, d = _SEGS[name]
        ref = CO.decode_soa(seg, CO.descs_array([tuple(int(x) for x in r) for r in d]), comp,
                            index_only)
        for v in ref.values():
            if v is not None:
                v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


# ---- one framed call ----------------------------------------------------------


class Call:
    """The framed inputs and outputs of one decode."""

    def __init__(self, dec, seg, d, comp, index_only, poison, base, cut=None):
        dev = _dev()
        kw = dict(base_mod=base, poison=poison, device=dev)
        self.dec, self.comp, self.index_only, self.n = dec, comp, index_only, d.shape[0]
        self.seg_bytes = len(seg)
        self.seg = G.frame_input(seg, **kw)
        self.descs = G.frame_input(d, np.uint64, **kw)
        r, k, v = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.flags = _lib.F_DEVICE_PTRS | (_lib.F_INDEX_ONLY if index_only else 0)
        rc = _lib.lib().okv_decode_plan(dec._ctx, self.seg.ptr, self.seg_bytes, self.descs.ptr,
                                        self.n, comp, self.flags, C.byref(r), C.byref(k),
                                        C.byref(v))
        assert rc == 0, dec.error()
        self.plan = (r.value, k.value, v.value)
        caps = dict(rows=r.value, key=k.value, val=v.value)
        caps.update(cut or {})
        self.caps = caps
        n = self.n
        self.out = {"row_start": G.frame(n + 1, np.uint64, **kw),
                    "key_base": G.frame(n, np.uint64, **kw),
                    "val_base": G.frame(n, np.uint64, **kw),
                    "status": G.frame(n, np.int32, **kw),
                    "key_arena": G.frame(caps["key"], np.uint8, **kw),
                    "val_arena": G.frame(caps["val"], np.uint8, **kw)}
        for name, dt in ROW_ARRAYS:  # all four row arrays have row_cap entries
            self.out[name] = G.frame(caps["rows"], dt, **kw)

    def decode_out(self, **ptrs):
        f = self.out
        p = {k: v.ptr for k, v in f.items()}
        p.update(ptrs)
        return _lib.DecodeOut(p["row_start"], p["key_base"], p["val_base"], p["status"],
                              p["key_off"], p["key_len"], p["val_off"], p["val_len"],
                              p["key_arena"], p["val_arena"], self.caps["rows"],
                              self.caps["key"], self.caps["val"], 0, 0, 0, 0)

    def run(self, extra_flags=0, seg_ptr=None, seg_bytes=None, **ptrs):
        self.o = self.decode_out(**ptrs)
        rc = _lib.lib().okv_decode_blocks(
            self.dec._ctx, self.seg.ptr if seg_ptr is None else seg_ptr,
            self.seg_bytes if seg_bytes is None else seg_bytes, self.descs.ptr, self.n,
            self.comp, C.byref(self.o), self.flags | extra_flags)
        return rc

    def guards(self):
        """G: every frame, inputs included."""
        self.seg.check("seg")
        self.descs.check("descs")
        for name, f in self.out.items():
            f.check(name)

    def outputs_untouched(self):
        """N."""
        for name, f in self.out.items():
            f.untouched(name)


def _assert_extents(c: Call, ref):
    """X: the extents the header defines equal the oracle, totals included."""
    n, full = c.n, not c.index_only
    h = {k: f.host() for k, f in c.out.items()}
    nr = int(ref["row_start"][-1])
    kb = ref["key_arena"].size if full else 0
    vb = ref["val_arena"].size if full else 0
    assert c.plan == (nr, kb, vb)
    assert (c.o.n_rows, c.o.key_bytes, c.o.val_bytes) == (nr, kb, vb)
    assert c.o.n_bad_blocks == int((ref["status"] != 0).sum())
    assert np.array_equal(h["status"], ref["status"])
    assert np.array_equal(h["row_start"], ref["row_start"])
    for name, _ in ROW_ARRAYS:
        assert h[name].size == nr and np.array_equal(h[name], ref[name]), name
    if full:
        assert np.array_equal(h["key_base"], ref["key_base"])
        assert np.array_equal(h["val_base"], ref["val_base"])
        for name in ("key_arena", "val_arena"):  # with the zero padding of every region
            bad = np.flatnonzero(h[name] != ref[name])
            assert not bad.size, (name, "first differing byte", int(bad[0]), "of", ref[name].size,
                                  "got", int(h[name][bad[0]]), "want", int(ref[name][bad[0]]))


# ---- G, X, D on every route ----------------------------------------------------


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("index_only", [False, True], ids=["full", "index"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_routes(request, route, index_only, poison, base):
    fixture, comp, want_path = ROUTES[route]
    dec = request.getfixturevalue(fixture)
    name, (seg, d) = _segment_of(route)
    ref = _ref_of(name, comp, index_only)
    c = Call(dec, seg, d, comp, index_only, poison, base)
    rc = c.run()
    c.guards()
    assert rc == 0, dec.error()
    if want_path is not None:
        assert dec.last_path() == want_path
    elif route in ("tile_edges", "crafted_large") and not index_only:
        assert dec.last_path() & _lib.PATH_TILE, dec.last_path()
    _assert_extents(c, ref)
    if index_only:  # no arenas exist: zero-length frames, nothing written near them
        c.out["key_arena"].untouched("key_arena")
        c.out["val_arena"].untouched("val_arena")


def test_route_segments_reach_past_seg_bytes():
    """D needs a read that really reaches past seg_bytes: these routes' segments
    end off a 16-byte boundary."""
    for route in ("fused", "no_fused", "fused_ragged", "tile_edges", "crafted_large"):
        _, (seg, _d) = _segment_of(route)
        assert len(seg) % 16 != 0, route


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
def test_async_tile(decoder, poison, base):
    """OKV_F_ASYNC on the tile route: okv_sync, then okv_decode_totals, then G and X."""
    name, (seg, d) = _segment_of("tile_big")
    ref = _ref_of(name, NONE, False)
    c = Call(decoder, seg, d, NONE, False, poison, base)
    rc = c.run(extra_flags=_lib.F_ASYNC)
    assert rc == 0, decoder.error()
    decoder.sync()
    assert _lib.lib().okv_decode_totals(decoder._ctx, C.byref(c.o)) == 0
    c.guards()
    assert decoder.last_path() == 68
    _assert_extents(c, ref)


# ---- capacity -------------------------------------------------------------------


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("amount", ["half", "zero"])
@pytest.mark.parametrize("cut", ["rows", "key", "val"])
@pytest.mark.parametrize("route", ["fused", "no_fused", "fused_ragged", "no_fused_ragged",
                                   "small_gather", "tile_big"])
def test_capacity(request, route, cut, amount, poison, base):
    """One capacity cut to about half, then to 0 (a pointer into the frame with
    no bytes behind it): G holds; the OKV_BLK_CAPACITY statuses are a suffix;
    every block before the first equals the oracle in full; the totals are the
    plan's."""
    fixture, comp, want_path = ROUTES[route]
    dec = request.getfixturevalue(fixture)
    name, (seg, d) = _segment_of(route)
    ref = _ref_of(name, comp, False)
    nr, kb, vb = int(ref["row_start"][-1]), ref["key_arena"].size, ref["val_arena"].size
    full = dict(rows=nr, key=kb, val=vb)[cut]
    # arenas are cut at a 16-byte multiple (their regions are), rows anywhere
    short = 0 if amount == "zero" else (full // 2 if cut == "rows" else full // 2 // 16 * 16 + 16)
    assert short < full
    c = Call(dec, seg, d, comp, False, poison, base, cut={cut: short})
    rc = c.run()
    c.guards()
    assert rc == _lib.OKV_E_CAPACITY, (rc, dec.error())
    assert dec.last_path() == want_path
    assert (c.o.n_rows, c.o.key_bytes, c.o.val_bytes) == (nr, kb, vb) == c.plan
    h = {k: f.host() for k, f in c.out.items()}
    st = h["status"]
    assert (st == _lib.BLK_CAPACITY).any()
    first_bad = int(np.argmax(st == _lib.BLK_CAPACITY))
    assert (st[first_bad:] == _lib.BLK_CAPACITY).all()  # a suffix
    assert np.array_equal(st[:first_bad], ref["status"][:first_bad])
    if amount == "half":
        assert first_bad > 0
    rs = ref["row_start"]
    kbase = np.append(ref["key_base"], np.uint64(kb))
    vbase = np.append(ref["val_base"], np.uint64(vb))
    for b in range(first_bad):
        r0, r1 = int(rs[b]), int(rs[b + 1])
        assert int(h["row_start"][b]) == r0 and int(h["row_start"][b + 1]) == r1
        assert int(h["key_base"][b]) == int(kbase[b]) and int(h["val_base"][b]) == int(vbase[b])
        for aname, _ in ROW_ARRAYS:
            assert np.array_equal(h[aname][r0:r1], ref[aname][r0:r1]), (b, aname)
        k0, k1, v0, v1 = int(kbase[b]), int(kbase[b + 1]), int(vbase[b]), int(vbase[b + 1])
        assert h["key_arena"][k0:k1].tobytes() == ref["key_arena"][k0:k1].tobytes(), b
        assert h["val_arena"][v0:v1].tobytes() == ref["val_arena"][v0:v1].tobytes(), b


# ---- misaligned bases -----------------------------------------------------------


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("which", ["seg", "key_arena", "val_arena"])
def test_misaligned_base_is_refused(decoder, which, poison, base):
    """base + 8 (inside the frame) for the segment or an output arena:
    OKV_E_ARG, and nothing is written."""
    name, (seg, d) = _segment_of("fused")
    c = Call(decoder, seg, d, NONE, False, poison, base)
    if which == "seg":
        rc = c.run(seg_ptr=c.seg.ptr + 8, seg_bytes=c.seg_bytes - 8)
    else:
        c.caps["key" if which == "key_arena" else "val"] -= 8
        rc = c.run(**{which: c.out[which].ptr + 8})
    assert rc == _lib.OKV_E_ARG
    c.guards()
    c.outputs_untouched()
