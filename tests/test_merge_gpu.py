"""Direct parity of the merge kernels (okv_merge_rows, objectkv_amd/csrc/
okv_merge.hip) at the edges of compare, rank and scan.

Inputs are built byte by byte as SoA tensors, no segment is written or
decoded.  OKV_MERGE_ALL is compared with a stable sort by (key bytes, stream)
written here; OKV_MERGE_GETRANGE with the restated Go loop over in-memory
streams (oracle.snapshot_oracle.merge_lists).  Every comparison is exact, and
every group asserts from the reference side that its inputs reach the branch it
names (long-key compare, the three rank forms, the scan block boundaries, the
five loop endings)."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest
import torch

import objectkv_amd as okv
from oracle import pyoracle as P
from oracle import snapshot_oracle as SO

pytestmark = pytest.mark.gpu

L = okv._lib
ASC, DESC = L.DIR_ASC, L.DIR_DESC
ALL, GETRANGE = L.MERGE_ALL, L.MERGE_GETRANGE
U64 = (1 << 64) - 1


# ---- inputs ----------------------------------------------------------------------------


class _At:
    """A device address inside a tensor (kept alive), where the wrapper expects
    a tensor."""

    def __init__(self, t, off):
        self.t, self.a = t, t.data_ptr() + off

    def data_ptr(self):
        return self.a


class Stream:
    """One merge input: host SoA (ko, kl, vo, vl), the six device tensors (.t),
    the arena addresses (.ka, .va), the level and the row range [lo, hi)."""

    def __init__(self, karena: np.ndarray, ko, kl, varena: np.ndarray, vo, vl, level=1, lo=0,
                 hi=None, align=0):
        dev = torch.device("cuda", 0)
        self.n = len(kl)
        self.ko, self.kl = np.asarray(ko, np.uint64), np.asarray(kl, np.uint16)
        self.vo, self.vl = np.asarray(vo, np.uint64), np.asarray(vl, np.uint32)
        # the key arena starts `align` bytes into a 16-byte line (allocations
        # are at least 16-byte aligned) and ends exactly at the last key byte
        kbuf = np.concatenate([np.zeros(align, np.uint8), karena])
        self._kbuf = torch.from_numpy(kbuf if kbuf.size else np.zeros(1, np.uint8)).to(dev)
        self._vbuf = torch.from_numpy(varena.copy() if varena.size
                                      else np.zeros(1, np.uint8)).to(dev)
        assert self._kbuf.data_ptr() % 16 == 0
        ka = _At(self._kbuf, align)

        def up(a, dt):
            a = np.ascontiguousarray(a).view(dt)
            return torch.from_numpy(a if a.size else np.zeros(1, dt)).to(dev)
        self.t = {"key_arena": ka, "key_off": up(self.ko, np.int64),
                  "key_len": up(self.kl, np.int16), "val_arena": self._vbuf,
                  "val_off": up(self.vo, np.int64), "val_len": up(self.vl, np.int32)}
        self.ka, self.va = ka.data_ptr(), self._vbuf.data_ptr()
        self.level, self.lo, self.hi = level, lo, self.n if hi is None else hi
        self.rows = None

    def src(self):
        return (self.t, self.lo, self.hi, self.level)


def stream_of_rows(rows, level=1, lo=0, hi=None, align=0) -> Stream:
    """rows: [(key bytes, value bytes or None)], strictly ascending by key."""
    assert all(a[0] < b[0] for a, b in zip(rows, rows[1:]))
    kl = [len(k) for k, _v in rows]
    vl = [len(v or b"") for _k, v in rows]
    ko = np.concatenate([[0], np.cumsum(kl)[:-1]]) if rows else []
    vo = np.concatenate([[0], np.cumsum(vl)[:-1]]) if rows else []
    s = Stream(np.frombuffer(b"".join(k for k, _v in rows), np.uint8), ko, kl,
               np.frombuffer(b"".join(v or b"" for _k, v in rows), np.uint8), vo, vl,
               level, lo, hi, align)
    s.rows = rows
    return s


def stream_of_u64(keys: np.ndarray, level=1) -> Stream:
    """Fixed 8-byte big-endian integer keys (strictly ascending), 1-byte values."""
    keys = np.asarray(keys, np.uint64)
    assert np.all(keys[1:] > keys[:-1])
    n = keys.size
    s = Stream(keys.astype(">u8").view(np.uint8), np.arange(n, dtype=np.uint64) * 8,
               np.full(n, 8, np.uint16), np.arange(251, dtype=np.uint8),
               np.arange(n, dtype=np.uint64) % 251, np.ones(n, np.uint32), level)
    s.keys = keys
    return s


# ---- the call --------------------------------------------------------------------------


class Result:
    pass


def run_merge(dec, streams, mode, direction, limit=0, bound=None, drop=False, soa=False,
              row_cap=None, key_base=None, val_base=None) -> Result:
    """okv_merge_rows through Decoder.merge_device -> rc, n_rows, n_unique,
    status, pairs [(src, row)] as an (n, 2) array, and with soa the four
    optional outputs."""
    dev = torch.device("cuda", 0)
    cap = sum(s.hi - s.lo for s in streams) if row_cap is None else row_cap
    a = max(cap, 1)
    out = {"src": torch.full((a,), -7, dtype=torch.int32, device=dev),
           "row": torch.full((a,), -7, dtype=torch.int64, device=dev)}
    if soa:
        out.update(key_off=torch.empty(a, dtype=torch.int64, device=dev),
                   key_len=torch.empty(a, dtype=torch.int16, device=dev),
                   val_off=torch.empty(a, dtype=torch.int64, device=dev),
                   val_len=torch.empty(a, dtype=torch.int32, device=dev))
    r = Result()
    r.rc = 0
    try:
        mo = dec.merge_device([s.src() for s in streams], mode, direction, limit, bound, drop,
                              out, key_base or 0, val_base or 0, cap)
    except okv.sst.OkvError as e:
        if e.code != L.OKV_E_CAPACITY:
            raise
        r.rc, mo = e.code, e.out
    r.n_rows, r.n_unique, r.status = int(mo.n_rows), int(mo.n_unique), int(mo.status)
    n = 0 if (r.rc or r.status) else r.n_rows
    r.pairs = np.stack([out["src"][:n].cpu().numpy().astype(np.int64),
                        out["row"][:n].cpu().numpy()], axis=1)
    if soa:
        r.soa = {k: out[k][:n].cpu().numpy() for k in ("key_off", "key_len", "val_off",
                                                      "val_len")}
    return r


def check_soa(r: Result, streams, key_base, val_base):
    """The optional outputs are the input rows' SoA entries, offsets rebased
    from each input's arena address onto key_base / val_base."""
    src, row = r.pairs[:, 0], r.pairs[:, 1]
    exp = {"key_off": [], "key_len": [], "val_off": [], "val_len": []}
    for s, q in zip(src.tolist(), row.tolist()):
        st = streams[s]
        exp["key_off"].append((st.ka - key_base + int(st.ko[q])) & U64)
        exp["key_len"].append(int(st.kl[q]))
        exp["val_off"].append((st.va - val_base + int(st.vo[q])) & U64)
        exp["val_len"].append(int(st.vl[q]))
    assert r.soa["key_off"].view(np.uint64).tolist() == exp["key_off"]
    assert r.soa["key_len"].view(np.uint16).tolist() == exp["key_len"]
    assert r.soa["val_off"].view(np.uint64).tolist() == exp["val_off"]
    assert r.soa["val_len"].view(np.uint32).tolist() == exp["val_len"]


# ---- references ------------------------------------------------------------------------


def ref_all(streams, direction, drop):
    """OKV_MERGE_ALL: stable sort by (key bytes, stream); the first row of each
    run owns the key; L0 owners with a nil value go when drop is set.
    -> ([(src, row)], n, n_unique)."""
    items = sorted((st.rows[q][0], s, q) for s, st in enumerate(streams)
                   for q in range(st.lo, st.hi))
    owners = [it for i, it in enumerate(items) if i == 0 or items[i - 1][0] != it[0]]
    rows = [(s, q) for _k, s, q in owners
            if not (drop and streams[s].level == 0 and streams[s].rows[q][1] is None)]
    if direction == DESC:
        rows.reverse()
    return rows, len(items), len(owners)


def ref_all_u64(streams, direction):
    """The same over stream_of_u64 inputs, as arrays: -> (pairs (nu, 2), n, nu)."""
    key = np.concatenate([s.keys for s in streams])
    src = np.concatenate([np.full(s.keys.size, i, np.int64) for i, s in enumerate(streams)])
    row = np.concatenate([np.arange(s.keys.size, dtype=np.int64) for s in streams])
    order = np.lexsort((src, key))
    k = key[order]
    first = np.ones(k.size, bool)
    first[1:] = k[1:] != k[:-1]
    pairs = np.stack([src[order][first], row[order][first]], axis=1)
    if direction == DESC:
        pairs = pairs[::-1]
    return pairs, int(key.size), int(first.sum())


def ref_getrange(streams, direction, bound, limit):
    """-> ([(src, row)] or None on io.EOF, how the loop ended)."""
    return SO.merge_lists([(s.rows, s.level, s.lo, s.hi) for s in streams], bound, limit,
                          P.DirectionDescending if direction == DESC else P.DirectionAscending)


def n_unique_of(streams):
    return len({s.rows[q][0] for s in streams for q in range(s.lo, s.hi)})


def check_all(dec, streams, direction, drop, soa=False):
    want, n, nu = ref_all(streams, direction, drop)
    kb = min(s.ka for s in streams) - 48 if soa else None
    vb = min(s.va for s in streams) if soa else None
    r = run_merge(dec, streams, ALL, direction, drop=drop, soa=soa, key_base=kb, val_base=vb)
    assert (r.rc, r.status, r.n_rows, r.n_unique) == (0, 0, len(want), nu)
    assert r.pairs.tolist() == [list(p) for p in want]
    if soa:
        check_soa(r, streams, kb, vb)
    return r


def check_getrange(dec, streams, direction, bound, limit, soa=False):
    want, end = ref_getrange(streams, direction, bound, limit)
    kb = min(s.ka for s in streams) if soa else None
    vb = min(s.va for s in streams) - 16 if soa else None
    r = run_merge(dec, streams, GETRANGE, direction, limit, bound, soa=soa, key_base=kb,
                  val_base=vb)
    assert r.rc == 0
    assert r.n_unique == n_unique_of(streams)
    if want is None:
        assert r.status == L.M_EOF, (end, r.n_rows)
    else:
        assert (r.status, r.n_rows) == (0, len(want)), end
        assert r.pairs.tolist() == [list(p) for p in want], end
        if soa:
            check_soa(r, streams, kb, vb)
    return end


# ---- a. long-key ordering --------------------------------------------------------------

P16 = bytes(range(0x41, 0x51))  # the 16 bytes every long-key family shares
DIFF_AT = (16, 17, 23, 24, 31, 32)
PREFIX_LENS = ((15, 16), (16, 17), (23, 24), (24, 25), (31, 33))
ZERO_LENS = (15, 16, 17, 24)
MAXKEY = 65535


def _long_key_families():
    fams = []
    for d in DIFF_AT:  # first difference at byte d, deciding bytes on both sides of 0x80
        head = P16 + bytes([0x10 + d]) * (d - 16)
        fams.append([head + bytes([x]) + b"tail" for x in (0x01, 0x7f, 0x80, 0xff)])
    body = P16 + b"\x55" * (MAXKEY - 17)
    fams.append([body + bytes([x]) for x in (0x00, 0x7f, 0x80)])  # last byte of a 65535-byte key
    for i, (a, b) in enumerate(PREFIX_LENS):  # one key a strict prefix of the other
        body = P16[:8] + bytes([0x88 + i]) * 25
        fams.append([body[:a], body[:b]])
    for i, n in enumerate(ZERO_LENS):  # keys that differ only by trailing zero bytes
        p = bytes([0x90 + i]) * n
        fams.append([p, p + b"\x00", p + b"\x00\x00"])
    return fams


def _first_diff(a, b):
    """Index of the first differing byte, or None when one is a prefix of the other."""
    m = min(len(a), len(b))
    if a[:m] == b[:m]:
        return None
    lo, hi = 0, m  # a[:lo] == b[:lo], a[:hi] != b[:hi]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if a[:mid] == b[:mid]:
            lo = mid
        else:
            hi = mid
    return lo


def _long_key_rows():
    """Four streams' row lists: every family spread over the streams, some keys
    in two streams, the empty key in streams 1 and 3."""
    per = [dict() for _ in range(4)]
    t = 0
    for fam in _long_key_families():
        for i, k in enumerate(sorted(fam)):
            for s in ((t + i) % 4,) + (((t + i + 1) % 4,) if i % 3 == 0 else ()):
                per[s][k] = None if (len(per[s]) % 5 == 2) else b"v%d-%d" % (s, len(per[s]))
        t += 1
    per[1][b""] = b"empty-1"
    per[3][b""] = None
    return [sorted(d.items()) for d in per]


def _long_key_precondition(rows):
    # precondition: cross-stream pairs decide at every named byte, by every
    # named prefix relation, and on bytes >= 0x80
    diffs, prefixes, high = set(), set(), set()
    keyed = [(k, s) for s, rs in enumerate(rows) for k, _v in rs]
    ties = 0
    for i, (a, sa) in enumerate(keyed):
        for b, sb in keyed[i + 1:]:
            if sa == sb:
                continue
            if a == b:
                ties += 1
                continue
            d = _first_diff(a, b)
            if d is None:
                prefixes.add((min(len(a), len(b)), max(len(a), len(b))))
            else:
                diffs.add(d)
                if max(a[d], b[d]) >= 0x80 and min(a[d], b[d]) < 0x80 and d >= 16:
                    high.add(d)
    assert set(DIFF_AT) | {MAXKEY - 1} <= diffs
    assert set(PREFIX_LENS) <= prefixes
    assert {(n, n + 1) for n in ZERO_LENS} | {(n, n + 2) for n in ZERO_LENS} <= prefixes
    assert set(DIFF_AT) | {MAXKEY - 1} <= high
    assert ties >= 8 and all(2 <= len(r) for r in rows)
    assert rows[1][0][0] == b"" and rows[3][0][0] == b""


@pytest.fixture(scope="module")
def long_key_rows():
    rows = _long_key_rows()
    _long_key_precondition(rows)
    return rows


@pytest.mark.parametrize("align", range(16))
def test_long_keys_merge_all(decoder, long_key_rows, align):
    """Keys equal in their first 16 bytes: the arena loop of key_cmp, the prefix
    tie-break past 16 bytes, trailing zero bytes, unsigned deciding bytes, the
    empty key; every byte alignment of the key arena."""
    streams = [stream_of_rows(rs, level=0 if s < 2 else 1, align=(align + 5 * s) % 16)
               for s, rs in enumerate(long_key_rows)]
    assert sorted(s.ka % 16 for s in streams) == sorted((align + 5 * s) % 16 for s in range(4))
    for direction in (ASC, DESC):
        for drop in (False, True):
            check_all(decoder, streams, direction, drop, soa=True)
    want, _n, _nu = ref_all(streams, ASC, False)
    assert want[0] == (1, 0)  # the empty key is the smallest and stream 1 owns it


@pytest.mark.parametrize("direction", [ASC, DESC])
def test_long_keys_getrange(decoder, long_key_rows, direction):
    """The same families (without the empty key) through the Go loop, bounds
    drawn from the long keys so the bound compare runs past 16 bytes too; once
    without tombstones (every level 1) and once with streams 0 and 1 on level 0."""
    rows = [[kv for kv in rs if kv[0]] for rs in long_key_rows]
    keys = sorted({k for rs in rows for k, _v in rs})
    assert sum(len(k) > 16 for k in keys) >= 30
    for levels in ((1, 1, 1, 1), (0, 0, 1, 2)):
        streams = [stream_of_rows(rs, level=levels[s], align=(3 + 5 * s) % 16)
                   for s, rs in enumerate(rows)]
        most = 0
        for bound in keys[::6] + [b"\xff", b""]:
            for limit in (3, 1 << 63):
                most = max(most, len(ref_getrange(streams, direction, bound, limit)[0] or []))
                check_getrange(decoder, streams, direction, bound, limit, soa=True)
        assert most >= 10 or levels[0] == 0  # precondition: long keys are compared and emitted


# ---- b. source count and empty inputs --------------------------------------------------


def _small_streams(seed, nsrc, shared=None):
    rng = random.Random(seed)
    pool = [b"key-%03d" % i for i in range(40)] + [P16 + b"-%02d" % i for i in range(10)]
    out = []
    for s in range(nsrc):
        ks = set(rng.sample(pool, rng.randint(1, 6)))
        if shared:
            ks.add(shared)
        level = 0 if s < nsrc // 2 else 1
        out.append([(k, None if level == 0 and k != shared and rng.random() < 0.2
                     else b"s%d" % s) for k in sorted(ks)])
    return out


@pytest.mark.parametrize("nsrc", [1, 2, 63, 64])
def test_source_counts(decoder, nsrc):
    shared = b"key-020-in-all"
    rows = _small_streams(nsrc, nsrc, shared)
    streams = [stream_of_rows(rs, level=0 if s < nsrc // 2 else 1, align=s % 16)
               for s, rs in enumerate(rows)]
    want, n, nu = ref_all(streams, ASC, False)
    own = [p for p in want if streams[p[0]].rows[p[1]][0] == shared]
    assert len(own) == 1 and own[0][0] == 0  # one key in every input: stream 0 owns it, once
    assert n - nu >= nsrc - 1
    for direction in (ASC, DESC):
        for drop in (False, True):
            check_all(decoder, streams, direction, drop)
        for bound, limit in ((b"\xff", 1 << 63), (b"", 1 << 63), (shared, 1000),
                             (b"key-030", 5)):
            check_getrange(decoder, streams, direction, bound, limit)


def test_empty_inputs(decoder):
    rows = _small_streams(9, 5)
    assert all(len(rs) >= 1 for rs in rows)
    for empty in ((0,), (2,), (4,), (0, 2, 4), (0, 1, 2, 3), (0, 1, 2, 3, 4)):
        streams = []
        for s, rs in enumerate(rows):
            at = min(1, len(rs))  # an empty range that is not [0, 0)
            lo, hi = (at, at) if s in empty else (0, len(rs))
            streams.append(stream_of_rows(rs, level=0 if s < 3 else 1, lo=lo, hi=hi))
        for direction in (ASC, DESC):
            r = check_all(decoder, streams, direction, True)
            check_getrange(decoder, streams, direction, b"\xff" if direction == ASC else b"",
                           1 << 63)
            check_getrange(decoder, streams, direction, b"key-020", 2)
            if len(empty) == 5:
                assert (r.n_rows, r.n_unique) == (0, 0)
    for mode in (ALL, GETRANGE):  # no inputs at all
        r = run_merge(decoder, [], mode, ASC, limit=1, bound=b"\xff")
        assert (r.rc, r.status, r.n_rows, r.n_unique) == (0, 0, 0, 0)


# ---- c. the three rank forms -----------------------------------------------------------

RANK_WIN = 1024  # kRankWin: staged window rows per workgroup


def _rank_forms(key_lists):
    """Per 256-row group of the global row numbering: ("straddle",) or
    ("one", window total, tie at the group's first row with an earlier stream,
    tie at its last row), as the rank kernel sees them."""
    sizes = [len(k) for k in key_lists]
    base = np.concatenate([[0], np.cumsum(sizes)])
    n = int(base[-1])
    out = []
    for g0 in range(0, n, 256):
        g1 = min(g0 + 256, n) - 1
        i0 = int(np.searchsorted(base, g0, "right")) - 1
        i1 = int(np.searchsorted(base, g1, "right")) - 1
        if i0 != i1:
            out.append(("straddle",))
            continue
        kf, kl = key_lists[i0][g0 - base[i0]], key_lists[i0][g1 - base[i0]]
        tot, tf, tl = 0, False, False
        for j, ks in enumerate(key_lists):
            if j == i0:
                continue
            side = "right" if j < i0 else "left"  # earlier streams own ties
            tot += int(np.searchsorted(ks, kl, side)) - int(np.searchsorted(ks, kf, side))
            if j < i0 and len(ks):
                tf |= bool(ks[min(np.searchsorted(ks, kf), len(ks) - 1)] == kf)
                tl |= bool(ks[min(np.searchsorted(ks, kl), len(ks) - 1)] == kl)
        out.append(("one", tot, tf, tl))
    return out


def _rank_cases():
    u = lambda x: np.asarray(x, np.uint64)  # noqa: E731
    t = np.arange(1024)
    edge = (t % 256 == 0) | (t % 256 == 255)
    rng = np.random.default_rng(17)
    pick = lambda n: np.sort(rng.choice(2000, n, replace=False))  # noqa: E731
    a5 = np.arange(512) * 5
    b5 = np.setdiff1d(np.arange(2560), a5)  # 4 keys in every gap of a5
    c5 = np.arange(103) * 25 + 1  # one more key in every 5th gap
    dense = np.arange(16 * 512)
    return {
        # equal density, K = 3: windows of a few hundred rows; stream 1 ties
        # stream 0 at the first and last row of each of its groups
        "equal": [u(2 * t), u(2 * t + np.where(edge, 0, 1)), u(3 * t)],
        # a sparse stream against one 16x denser over the same range: 4080-row windows
        "sparse-first": [u(dense[::16]), u(dense)],
        "sparse-last": [u(dense), u(dense[::16])],  # every sparse key is owned by the dense one
        "win-1020": [u(a5), u(b5)],
        "win-1071": [u(a5), u(b5), u(c5)],
        "straddle-2": [u(pick(n)) for n in (1, 255, 257, 300, 1)],
        "straddle-3": [u(pick(n)) for n in (100, 50, 300)],
    }


def _rank_precondition(cases):
    forms = {name: _rank_forms(ks) for name, ks in cases.items()}
    allf = [f for fs in forms.values() for f in fs]
    one = [f for f in allf if f[0] == "one"]
    # precondition: all three forms, both sides of the staging limit within 64
    # rows, and staged groups whose first / last row ties an earlier stream
    assert any(f[1] <= RANK_WIN for f in one)
    assert any(f[1] > RANK_WIN for f in one)
    assert any(f[0] == "straddle" for f in allf)
    assert any(RANK_WIN - 64 <= f[1] <= RANK_WIN for f in one)
    assert any(RANK_WIN < f[1] <= RANK_WIN + 64 for f in one)
    assert any(f[1] <= RANK_WIN and f[2] for f in one)
    assert any(f[1] <= RANK_WIN and f[3] for f in one)
    assert any(f[1] > RANK_WIN and f[2] and f[3] for f in one)
    assert all(f[1] >= 8 * 255 for f in forms["sparse-first"][:2])
    assert sum(f[0] == "straddle" for f in forms["straddle-2"]) == 3
    assert forms["straddle-2"][1][0] == "one" and forms["straddle-3"][0] == ("straddle",)


@pytest.fixture(scope="module")
def rank_cases():
    cases = _rank_cases()
    _rank_precondition(cases)
    return cases


@pytest.mark.parametrize("name", ["equal", "sparse-first", "sparse-last", "win-1020", "win-1071",
                                  "straddle-2", "straddle-3"])
def test_rank_forms(decoder, rank_cases, name):
    streams = [stream_of_u64(k) for k in rank_cases[name]]
    for direction in (ASC, DESC):
        want, n, nu = ref_all_u64(streams, direction)
        r = run_merge(decoder, streams, ALL, direction)
        assert (r.rc, r.status, r.n_rows, r.n_unique) == (0, 0, nu, nu)
        assert np.array_equal(r.pairs, want)


# ---- d. scan boundaries ----------------------------------------------------------------

SCAN_EDGES = (4095, 4096, 4097, 8192, 8193)
SCAN_PAIRS = ((4095, 4095), (4096, 4095), (4096, 4096), (4097, 4096), (4097, 4097),
              (8192, 4097), (8192, 8192), (8193, 8192), (8193, 8193), (8193, 4097))
assert {a for a, _b in SCAN_PAIRS} == set(SCAN_EDGES) == {b for _a, b in SCAN_PAIRS}


def _scan_streams(n, nu):
    """Three streams with n rows and nu distinct keys: the keys split between
    streams 0 and 1, and n - nu of them repeated in stream 2."""
    keys = np.arange(nu, dtype=np.uint64) * 3 + 7
    d = n - nu
    assert 0 <= d <= nu
    dup = keys[np.linspace(0, nu - 1, d).astype(np.int64)] if d else keys[:0]
    return [keys[0::2], keys[1::2], np.unique(dup)]


@pytest.mark.parametrize("n1,nu1", SCAN_PAIRS)
def test_scan_boundaries(decoder, n1, nu1):
    """n + 1 owner flags and nu + 1 emit flags on both sides of one and two
    4096-element scan blocks."""
    streams = [stream_of_u64(k) for k in _scan_streams(n1 - 1, nu1 - 1)]
    for direction in (ASC, DESC):
        want, n, nu = ref_all_u64(streams, direction)
        assert (n + 1, nu + 1) == (n1, nu1)  # precondition
        r = run_merge(decoder, streams, ALL, direction)
        assert (r.rc, r.status, r.n_rows, r.n_unique) == (0, 0, nu, nu)
        assert np.array_equal(r.pairs, want)


def test_scan_carry_across_sums_pass(decoder):
    """More than 4096 * 1024 flags in both scans: the block-sums kernel takes a
    second 1024-block pass and must carry the first pass's total into it."""
    rng = np.random.default_rng(5)
    nu, ties = 4096 * 1024 + 700, 3000
    u = np.unique(rng.integers(0, 1 << 63, size=nu + 4096, dtype=np.uint64))[:nu]
    assert u.size == nu
    to = rng.integers(0, 4, size=nu)
    parts = [u[to == s] for s in range(4)]
    again = parts[0][:: parts[0].size // ties][:ties]  # stream 0's keys repeated in stream 2
    parts[2] = np.sort(np.concatenate([parts[2], again]))
    streams = [stream_of_u64(k) for k in parts]
    want, n, got_nu = ref_all_u64(streams, ASC)
    assert n == nu + ties and got_nu == nu  # precondition
    assert (n + 1 + 4095) // 4096 > 1024 and (nu + 1 + 4095) // 4096 > 1024
    r = run_merge(decoder, streams, ALL, ASC)
    assert (r.rc, r.status, r.n_rows, r.n_unique) == (0, 0, nu, nu)
    assert np.array_equal(r.pairs, want)


# ---- e. GETRANGE against the Go loop ---------------------------------------------------

GR_CASES = 360
GR_LIMITS = (1, 2, 3, 7, 1000, 1 << 63)
GR_POOL = sorted({b"k%02d" % i for i in range(44)} |
                 {P16 + s for s in (b"", b"\x00", b"\x00\x00", b"x", b"xy", b"xyzzy123",
                                    b"xyzzy124", b"xyzzy124\x00", b"\x80", b"\x80\x80" * 9)} |
                 {b"a", b"ab", b"abcdefghijklmnop", b"abcdefghijklmnopq", b"z" * 40, b"\xfe",
                  b"\xff", b"\xff\x01"})


def _getrange_case(seed):
    rng = random.Random(seed)
    streams = []
    for _ in range(rng.randint(1, 6)):
        level = rng.choice((0, 0, 0, 1, 2))
        ks = sorted(rng.sample(GR_POOL, rng.randint(1, 40)))
        rows = [(k, None if rng.random() < (0.2 if level == 0 else 0.04)
                 else b"v-" + k[:6]) for k in ks]
        lo, hi = 0, len(rows)
        if rng.random() < 0.3:
            lo = rng.randrange(0, len(rows))
            hi = rng.randint(lo + 1, len(rows))
            if rng.random() < 0.1:
                hi = lo
        if level == 0 and hi > lo and rng.random() < 0.3:
            # a stream that runs out on a tombstone, at either end: both io.EOF
            # forms need one, and 20 % of rows alone rarely puts one there
            for q in (lo, hi - 1):
                rows[q] = (rows[q][0], None)
        streams.append((rows, level, lo, hi))
    direction = rng.choice((ASC, DESC))
    bound = rng.choice(GR_POOL + [b"\xff", b""] * 4)
    return streams, direction, bound, rng.choice(GR_LIMITS)


def _getrange_precondition(cases):
    ends = {}
    for streams, direction, bound, limit in cases:
        _rows, end = SO.merge_lists(
            streams, bound, limit,
            P.DirectionDescending if direction == DESC else P.DirectionAscending)
        ends[end] = ends.get(end, 0) + 1
    # precondition: the reference loop ends in all five ways over this set
    for e in (SO.END_LIMIT, SO.END_BOUND, SO.END_STALE, SO.END_EOF_ROLL, SO.END_EOF_STALE):
        assert ends.get(e, 0) >= 3, ends
    assert any(len(k) > 16 for ss, _d, _b, _l in cases for rs, _lv, _lo, _hi in ss
               for k, _v in rs)
    return ends


@pytest.fixture(scope="module")
def getrange_cases():
    cases = [_getrange_case(1000 + i) for i in range(GR_CASES)]
    _getrange_precondition(cases)
    return cases


@pytest.mark.parametrize("part", range(6))
def test_getrange_random(decoder, getrange_cases, part):
    for i, (ss, direction, bound, limit) in enumerate(getrange_cases):
        if i % 6 != part:
            continue
        streams = [stream_of_rows(rows, level, lo, hi, align=(i + 7 * s) % 16)
                   for s, (rows, level, lo, hi) in enumerate(ss)]
        check_getrange(decoder, streams, direction, bound, limit, soa=True)


def _kv(*keys):
    """b"k3" -> live row, b"k3!" -> nil value (a tombstone on level 0)."""
    return [(k.rstrip(b"!"), None if k.endswith(b"!") else b"v" + k) for k in keys]


# (streams [(rows, level)], direction, bound, limit) -> how the Go loop ends
TERMINATION_TIES = {
    # the limit-th emit is also the key a stream runs out on: the limit wins
    "limit-on-stale-key": ([(_kv(b"k1", b"k2"), 1), (_kv(b"k1", b"k2", b"k3"), 1)],
                           ASC, b"\xff", 2, SO.END_LIMIT, 2),
    "stale-without-limit": ([(_kv(b"k1", b"k2"), 1), (_kv(b"k1", b"k2", b"k3"), 1)],
                            ASC, b"\xff", 3, SO.END_STALE, 2),
    # ... and the stream that ran out stands on an L0 tombstone: the limit
    # still wins, one more row and it is io.EOF
    "limit-on-stale-tombstone": ([(_kv(b"k1", b"k2", b"k3"), 0), (_kv(b"k2!"), 0)],
                                 ASC, b"\xff", 2, SO.END_LIMIT, 2),
    "stale-tombstone": ([(_kv(b"k1", b"k2", b"k3"), 0), (_kv(b"k2!"), 0)],
                        ASC, b"\xff", 3, SO.END_EOF_STALE, None),
    # a stop after k2 and a bound break before k3 share a position: the stop first
    "stale-then-bound": ([(_kv(b"k1", b"k2", b"k3"), 1), (_kv(b"k2"), 1)],
                         ASC, b"k3", 9, SO.END_STALE, 2),
    "stale-tombstone-then-bound": ([(_kv(b"k1", b"k2", b"k3"), 0), (_kv(b"k2!"), 0)],
                                   ASC, b"k3", 9, SO.END_EOF_STALE, None),
    "limit-then-bound": ([(_kv(b"k1", b"k2", b"k3"), 1)], ASC, b"k3", 2, SO.END_LIMIT, 2),
    # a tombstone past the bound whose stream runs out: the break at k3 comes first
    "bound-before-eof": ([(_kv(b"k1", b"k3", b"k9"), 1), (_kv(b"k5!"), 0)],
                         ASC, b"k2", 9, SO.END_BOUND, 1),
    # the tombstone is the first key past the bound: it is rolled before the range check
    "eof-at-bound": ([(_kv(b"k1", b"k9"), 1), (_kv(b"k5!"), 0)],
                     ASC, b"k2", 9, SO.END_EOF_ROLL, None),
    "bound-before-eof-desc": ([(_kv(b"k1", b"k5", b"k9"), 1), (_kv(b"k3!"), 0)],
                              DESC, b"k6", 9, SO.END_BOUND, 1),
    "eof-at-bound-desc": ([(_kv(b"k1", b"k9"), 1), (_kv(b"k3!"), 0)],
                          DESC, b"k6", 9, SO.END_EOF_ROLL, None),
    "stale-desc": ([(_kv(b"k2", b"k3"), 1), (_kv(b"k1", b"k2", b"k3"), 1)],
                   DESC, b"", 9, SO.END_STALE, 2),
}


@pytest.mark.parametrize("name", sorted(TERMINATION_TIES))
def test_getrange_termination_order(decoder, name):
    ss, direction, bound, limit, want_end, want_rows = TERMINATION_TIES[name]
    streams = [stream_of_rows(rows, level) for rows, level in ss]
    rows, end = ref_getrange(streams, direction, bound, limit)
    # precondition: the reference ends this case the way its name says
    assert end == want_end and (rows is None if want_rows is None else len(rows) == want_rows)
    assert check_getrange(decoder, streams, direction, bound, limit, soa=True) == want_end


# ---- f. capacity, reuse and arguments --------------------------------------------------


@pytest.mark.parametrize("mode", [ALL, GETRANGE])
def test_row_capacity(decoder, mode):
    rows = _small_streams(3, 4)
    streams = [stream_of_rows(rs, level=1) for rs in rows]
    if mode == ALL:
        want, _n, nu = ref_all(streams, ASC, False)
    else:
        want, end = ref_getrange(streams, ASC, b"\xff", 1 << 63)
        nu = n_unique_of(streams)
    assert len(want) >= 3
    r = run_merge(decoder, streams, mode, ASC, 1 << 63, b"\xff", row_cap=len(want) - 1)
    assert (r.rc, r.n_rows, r.n_unique) == (L.OKV_E_CAPACITY, len(want), nu)
    r = run_merge(decoder, streams, mode, ASC, 1 << 63, b"\xff", row_cap=len(want))
    assert (r.rc, r.status, r.n_rows) == (0, 0, len(want))
    assert r.pairs.tolist() == [list(p) for p in want]


def test_scratch_reuse_after_larger_call():
    """200 000 rows, then 10, then 300 000 on one fresh context: the scratch
    grows twice, and the small call runs over buffers (and their mown[n] /
    escan[nu] pads) that the larger one left full."""
    dec = okv.Decoder(0)
    try:
        rng = np.random.default_rng(23)
        for n in (200_000, 10, 300_000):
            parts = [np.unique(rng.integers(0, 2 * n, size=n, dtype=np.uint64))
                     [: n // 3 + (1 if s < n % 3 else 0)] for s in range(3)]
            streams = [stream_of_u64(k) for k in parts]
            for direction in (ASC, DESC):
                want, got_n, nu = ref_all_u64(streams, direction)
                assert got_n == n and nu <= got_n
                r = run_merge(dec, streams, ALL, direction)
                assert (r.rc, r.status, r.n_rows, r.n_unique) == (0, 0, nu, nu)
                assert np.array_equal(r.pairs, want)
    finally:
        dec.close()


def _getrange_walk_rows(seed, nsrc, n):
    """nsrc streams of n rows: 9-digit keys drawn from one range (so the
    streams share some keys and all end near the range's end), short values."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(nsrc):
        ks = np.unique(rng.integers(0, 3 * nsrc * n, size=n + n // 4 + 8))[:n]
        assert ks.size == n
        out.append([(b"%09d" % k, b"v%d" % s) for k in ks.tolist()])
    return out


def test_getrange_scratch_grows_and_is_reused():
    """One context walked through grow and reuse of the merge scratch
    (okv::Buf): a GETRANGE of 2 streams x 100 rows, then 8 streams x 20 000
    rows (40 scan blocks of 4096: every per-row array, the block sums and the
    rank windows grow), then the first again over the buffers the larger call
    left full -- each equal to the Go loop's rows."""
    small = [stream_of_rows(rs, level=1) for rs in _getrange_walk_rows(61, 2, 100)]
    large = [stream_of_rows(rs, level=1) for rs in _getrange_walk_rows(62, 8, 20_000)]
    assert (sum(s.hi - s.lo for s in large) + 1 + 4095) // 4096 > 1
    dec = okv.Decoder(0)
    try:
        for streams in (small, large, small):
            end = check_getrange(dec, streams, ASC, b"\xff", 1 << 63, soa=True)
            assert end == SO.END_STALE
    finally:
        dec.close()


def _raw_call(dec, streams, nsrc=None, flags=L.F_DEVICE_PTRS, mode=GETRANGE, direction=ASC,
              limit=1, bound=b"k", bound_len=None, ranges=None):
    nsrc = len(streams) if nsrc is None else nsrc
    arr = (L.MergeSrc * max(1, nsrc))()
    for i in range(nsrc):
        s = streams[i % len(streams)]
        lo, hi = ranges[i] if ranges else (s.lo, s.hi)
        t = s.t
        arr[i] = L.MergeSrc(t["key_arena"].data_ptr(), t["key_off"].data_ptr(),
                            t["key_len"].data_ptr(), t["val_arena"].data_ptr(),
                            t["val_off"].data_ptr(), t["val_len"].data_ptr(), lo, hi, s.level, 0)
    b = None if bound is None else np.frombuffer(bytes(bound), np.uint8)
    opts = L.MergeOpts(mode, direction, 0, 0, limit, None if b is None else b.ctypes.data,
                       (0 if b is None else b.size) if bound_len is None else bound_len)
    mo = L.MergeOut(None, None, None, None, None, None, None, None, 0, 0, 0, 0, 0)
    return L.lib().okv_merge_rows(dec._ctx, arr, nsrc, C.byref(opts), C.byref(mo), flags), mo


def test_argument_errors(decoder):
    streams = [stream_of_rows(_kv(b"k1", b"k2"), 1), stream_of_rows(_kv(b"k2", b"k3"), 1)]
    assert ref_getrange(streams, ASC, b"k3", 9)[0] == [(0, 0), (0, 1)]
    # the call shape is valid: with no output capacity it reports the two rows
    rc, mo = _raw_call(decoder, streams, bound=b"k3", limit=9)
    assert (rc, mo.n_rows, mo.n_unique) == (L.OKV_E_CAPACITY, 2, 3)
    long_bound = bytes(0x10000)
    bad = {
        "no OKV_F_DEVICE_PTRS": dict(flags=0),
        "mode": dict(mode=2),
        "direction": dict(direction=2),
        "limit 0": dict(limit=0),
        "null bound": dict(bound=None, bound_len=3),
        "bound_len > 0xffff": dict(bound=long_bound),
        "row_hi < row_lo": dict(ranges=[(0, 2), (2, 1)]),
        "65 inputs": dict(nsrc=65),
    }
    for what, kw in bad.items():
        rc, _mo = _raw_call(decoder, streams, **kw)
        assert rc == L.OKV_E_ARG, what
    for what in ("direction", "row_hi < row_lo", "65 inputs", "no OKV_F_DEVICE_PTRS"):
        rc, _mo = _raw_call(decoder, streams, mode=ALL, **bad[what])
        assert rc == L.OKV_E_ARG, what
    rc, mo = _raw_call(decoder, streams, nsrc=64, bound=b"k3", limit=9)  # 64 is accepted
    assert (rc, mo.n_rows, mo.n_unique) == (L.OKV_E_CAPACITY, 2, 3)
