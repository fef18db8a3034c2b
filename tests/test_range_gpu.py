"""Range reads from resident segments on the GPU: okv_seek_rows against pyoracle's RowIter
(tests/seek_cases.py), okv_gather_rows against numpy, snapshot.Reader.GetRanges and the
resident RowIter against oracle/snapshot_oracle.py, and the cost of a page
(Reader.range_stats)."""
from __future__ import annotations

import random

import numpy as np
import pytest

from objectkv_amd import _lib
from objectkv_amd import range as RG
from objectkv_amd import snapshot as SN
from objectkv_amd.sst import OkvError, fetch_metadata
from oracle import pyoracle as P
from oracle import snapshot_oracle as SO
from tests import seek_cases as SK
from tests import snapshot_cases as SC

pytestmark = pytest.mark.gpu
ASC, DESC = P.DirectionAscending, P.DirectionDescending


def _dev(a, dt=None):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(dt) if dt is not None else a.copy())
    return t.to(torch.device("cuda", 0))


# ---- okv_seek_rows -------------------------------------------------------------------


@pytest.fixture(scope="module")
def seek_world():
    """The seek cases' segments as device sources built by hand (keys back to back with
    ARENA_SPARE bytes after them), and every (source, key, direction, lo, hi)."""
    sources, keep, triples = [], [], []
    for s, (_name, keys, first, qs) in enumerate(SK.cases()):
        arena = np.frombuffer(b"".join(keys) + bytes(RG.ARENA_SPARE), np.uint8)
        kl = np.array([len(k) for k in keys], np.uint16)
        ko = np.concatenate([[0], np.cumsum(kl[:-1], dtype=np.uint64)]).astype(np.uint64)
        t = [_dev(arena), _dev(ko, np.int64), _dev(kl, np.int16),
             _dev(np.array(first, np.uint64), np.int64)]
        keep.append(t)
        sources.append(_lib.SeekSrc(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                    t[3].data_ptr(), len(keys), len(first) - 1))
        triples += [(s, q, d, lo, hi) for q, d, lo, hi in qs]
    random.Random(5).shuffle(triples)  # several sources in every batch
    return sources, keep, triples


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_seek_rows_against_row_iter(decoder, seek_world, n):
    from objectkv_amd.bloom import pack_keys
    sources, _keep, triples = seek_world
    assert len(triples) >= 257
    for at in (0, len(triples) - n):
        batch = triples[at:at + n]
        assert n < 3 or len({b[0] for b in batch}) > 1
        keys = [b[1] for b in batch]
        src_of, dirs = [b[0] for b in batch], [b[2] for b in batch]
        want = ([b[3] for b in batch], [b[4] for b in batch])
        lo, hi = RG.seek_rows(decoder, sources, keys, src_of, dirs)  # host mode
        assert (lo.tolist(), hi.tolist()) == want
        k = pack_keys(keys)
        dk = {"key_arena": _dev(np.concatenate([k["key_arena"], np.zeros(16, np.uint8)])),
              "key_off": _dev(k["key_off"], np.int64), "key_len": _dev(k["key_len"], np.int16)}
        out = {"row_lo": _dev(np.full(n, -1, np.int64)), "row_hi": _dev(np.full(n, -1, np.int64))}
        RG.seek_rows(decoder, sources, dk, _dev(np.array(src_of, np.int32)),
                     _dev(np.array(dirs, np.uint8)), out=out, n_rows=n)  # device mode
        assert (out["row_lo"].cpu().tolist(), out["row_hi"].cpu().tolist()) == want


def test_seek_rows_empty_batch_and_bad_source(decoder, seek_world):
    sources, _keep, _t = seek_world
    lo, hi = RG.seek_rows(decoder, sources, [], [], [])
    assert lo.size == 0 and hi.size == 0
    with pytest.raises(OkvError) as e:
        RG.seek_rows(decoder, sources, [b"k"], [len(sources)], [ASC])
    assert e.value.code == _lib.OKV_E_ARG


# ---- okv_gather_rows ------------------------------------------------------------------

VAL_LENS = (0, 1, 15, 16, 17, 4097)
KEY_LENS = (1, 16, 17)


def _gather_rows():
    """Rows with every value and key length the gather has to get right, ascending, with
    fillers of every length 0 .. 15 so that the offsets take every misalignment."""
    rng = random.Random(3)
    rows, i = [], 0
    for rep in range(3):
        for kl in KEY_LENS:
            for vl in VAL_LENS:
                k = (b"%c" % (65 + i // 200) + b"%03d" % (i % 200) + b"x" * 20)[:kl] if kl > 1 \
                    else None
                rows.append((k, bytes(rng.getrandbits(8) for _ in range(vl))))
                i += 1
        for pad in range(16):
            rows.append((b"f%03d" % i, bytes(rng.getrandbits(8) for _ in range(pad))))
            i += 1
    # 1-byte keys: the three that sort first
    ones = iter([b"\x01", b"\x02", b"\x03", b"\x04", b"\x05", b"\x06", b"\x07", b"\x08", b"\x09",
                 b"\x0a", b"\x0b", b"\x0c", b"\x0d", b"\x0e", b"\x0f", b"\x10", b"\x11", b"\x12"])
    rows = [(next(ones) if k is None else k, v) for k, v in rows]
    return sorted(set(rows), key=lambda r: r[0])


@pytest.fixture(scope="module")
def gather_world(decoder):
    """Two resident sources -- an uncompressed segment (index-only over its raw bytes) and a
    zstd segment (arenas) -- and their rows on the host."""
    from oracle import zstd_ref as Z
    rows = _gather_rows()
    assert len({k for k, _ in rows}) == len(rows)
    w = P.SegmentWriter(P.SegmentWriterOptions())
    for k, v in rows:
        w.WriteRow(k, v)
    n, _meta = w.Close()
    raw = bytes(w.external)
    zrows = [(b"z" + k, v[::-1]) for k, v in rows]
    zseg, zn, _ = Z.zstd_segment(zrows, 3584, 4096, level=3)
    res = []
    for data, flen in ((raw, n), (zseg, zn)):
        a = np.frombuffer(data, np.uint8)
        t = _dev(np.concatenate([a, np.zeros(RG.ARENA_SPARE, np.uint8)]))
        r = RG.ResidentRows(decoder, t, a.size, fetch_metadata(a, flen))
        assert not r.status.any()
        res.append(r)
    assert res[0].index_only and not res[1].index_only
    assert res[0].n == len(rows) and res[1].n == len(rows)
    vo = res[0].t["val_off"].cpu().numpy()
    ko = res[0].t["key_off"].cpu().numpy()
    assert {int(x) & 15 for x in vo} == set(range(16)) and {int(x) & 15 for x in ko} == set(range(16))
    return res, [rows, zrows]


def _check_gather(g, picks, host_rows):
    kpos = vpos = 0
    for i, (s, r) in enumerate(picks):
        k, v = host_rows[s][r]
        assert int(g.key_pos[i]) == kpos and int(g.val_pos[i]) == vpos, i
        assert int(g.key_len[i]) == len(k) and int(g.val_len[i]) == len(v), i
        pk, pv = -len(k) % 16, -len(v) % 16
        assert g.key_arena[kpos:kpos + len(k) + pk].tobytes() == k + bytes(pk), i
        assert g.val_arena[vpos:vpos + len(v) + pv].tobytes() == v + bytes(pv), i
        assert g.key(i) == k and g.value(i) == (v if v else None)
        kpos += len(k) + pk
        vpos += len(v) + pv
    assert (g.key_bytes, g.val_bytes) == (kpos, vpos)


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_gather_rows_against_numpy(decoder, gather_world, n):
    res, host_rows = gather_world
    rng = random.Random(n)
    nrows = len(host_rows[0])
    picks = [(rng.randrange(2), rng.randrange(nrows)) for _ in range(n)]
    src = _dev(np.array([p[0] for p in picks] + [0], np.int32))
    row = _dev(np.array([p[1] for p in picks] + [0], np.int64))
    g = RG.gather_rows(decoder, res, src, row, n)  # host mode: the size query, then the rows
    _check_gather(g, picks, host_rows)


def test_gather_rows_every_row_device_mode_and_capacity(decoder, gather_world):
    import torch
    res, host_rows = gather_world
    nrows = len(host_rows[0])
    picks = [(s, r) for r in range(nrows) for s in (0, 1)]
    lens = {len(host_rows[s][r][1]) for s, r in picks}
    assert set(VAL_LENS) <= lens and {len(host_rows[0][r][0]) for r in range(nrows)} >= set(KEY_LENS)
    n = len(picks)
    src = _dev(np.array([p[0] for p in picks], np.int32))
    row = _dev(np.array([p[1] for p in picks], np.int64))
    size = RG.gather_rows(decoder, res, src, row, n, arenas=False)  # the size query alone
    assert size.key_bytes > 0 and size.val_bytes > 3 * 4097
    dev = src.device

    def outs(kc, vc):
        return {"key_pos": torch.zeros(n, dtype=torch.int64, device=dev),
                "key_len": torch.zeros(n, dtype=torch.int16, device=dev),
                "val_pos": torch.zeros(n, dtype=torch.int64, device=dev),
                "val_len": torch.zeros(n, dtype=torch.int32, device=dev),
                "key_arena": torch.full((kc,), 0xAB, dtype=torch.uint8, device=dev),
                "val_arena": torch.full((vc,), 0xAB, dtype=torch.uint8, device=dev)}
    for kc, vc in ((size.key_bytes - 16, size.val_bytes), (size.key_bytes, size.val_bytes - 16)):
        o = outs(kc, vc)
        with pytest.raises(OkvError) as e:  # too small: the totals are set, nothing is written
            RG.gather_rows(decoder, res, src, row, n, out=o)
        assert e.value.code == _lib.OKV_E_CAPACITY
        assert (e.value.result.key_bytes, e.value.result.val_bytes) == (size.key_bytes, size.val_bytes)
        assert bool((o["key_arena"] == 0xAB).all()) and bool((o["val_arena"] == 0xAB).all())
        assert o["key_len"].cpu().numpy().view(np.uint16).tolist() == \
            [len(host_rows[s][r][0]) for s, r in picks]
    o = outs(size.key_bytes, size.val_bytes)
    g = RG.gather_rows(decoder, res, src, row, n, out=o)
    host = {k: o[k].cpu().numpy().view(t) for k, t in RG._GATHER}
    _check_gather(RG.GatherResult(host, o["key_arena"].cpu().numpy(), o["val_arena"].cpu().numpy(), g),
                  picks, host_rows)


# ---- Reader.GetRanges ----------------------------------------------------------------


def _pair(segs, decoder):
    data = {sid: (d, n) for sid, _l, d, n, _m in segs}
    orc = SO.Reader(lambda rec: P.SegmentReader(*data[rec.ID]))
    dev = SN.Reader(lambda rec: data[rec.ID], decoder)
    orecs, drecs = [], []
    for sid, lvl, _d, _n, meta in segs:
        md = P.bytes_to_metadata(meta)
        orecs.append(SO.SegmentRecord(sid, lvl, md.FirstKey, md.LastKey))
        drecs.append(SN.SegmentRecord(sid, lvl, md.FirstKey, md.LastKey))
    orc.UpdateSegments(orecs, None)
    dev.UpdateSegments(drecs, None)
    return orc, dev


def _outcome(fn):
    try:
        rows = fn()
    except (P.GoError, SN.SnapshotError) as e:
        return ("err", e.kind)
    except (P.GoPanic, SN.SnapshotPanic):
        return ("panic",)
    if rows is None:
        return ("nil",)
    return ("rows", [(r.Key, r.Value) for r in rows])


def _returned(x):
    def fn():
        if isinstance(x, Exception):
            raise x
        return x
    return _outcome(fn)


def _same_ranges(orc, dev, queries):
    """All queries in one GetRanges call against the oracle's GetRange of each."""
    got = dev.GetRanges(queries)
    assert len(got) == len(queries)
    outs = []
    for q, g in zip(queries, got):
        want = _outcome(lambda: orc.GetRange(*q))
        assert _returned(g) == want, (q, _returned(g), want)
        outs.append(want)
    st = dev.range_stats
    assert set(st) == set(SN._RANGE_STATS) and st["seek_calls"] <= 1
    return outs


def test_get_ranges_reference_snapshot(decoder):
    orc, dev = _pair(SC.reference_segments(), decoder)
    calls = [(b"key000", b"key006", 100), (b"key000", b"key006", 2), (b"key010", b"key106", 10),
             (b"key00", b"key0000", 2), (b"key000", b"key0000", 2), (b"key900", b"key901", 2),
             (b"key901", b"key910", 100), (b"key00", b"key000", 2), (b"key899", b"key901", 2),
             (b"key190", P.UnboundEnd, 100), (P.UnboundStart, b"key050", 1000),
             (b"key006", b"key000", 5), (b"key000", b"key006", 0)]
    queries = [(s, e, lim, d) for d in (ASC, DESC) for s, e, lim in calls]
    outs = _same_ranges(orc, dev, queries)
    assert {o[0] for o in outs} >= {"rows", "err", "panic"}
    assert dev.range_stats["seek_calls"] == 1 and dev.range_stats["gather_calls"] >= 1
    assert dev.GetRanges([]) == [] and dev.range_stats["seek_calls"] == 0
    rows = dev.GetRanges([(b"key000", b"key006", 100, ASC)])[0]
    assert [r.Key for r in rows] == [b"key000", b"key001", b"key0010", b"key002", b"key003",
                                     b"key004", b"key005"]
    assert _returned(dev.GetRanges([(b"k", b"l", -1, ASC)])[0]) == ("panic",)


@pytest.mark.parametrize("seed", range(6))
def test_get_ranges_random_snapshot(decoder, seed):
    segs, keys = SC.random_snapshot(seed, nseg=3 + seed % 4)
    orc, dev = _pair(segs, decoder)
    rng = random.Random(100 + seed)
    probes = keys + [k + b"\x00" for k in keys[::7]] + [b"", b"k", b"z", P.UnboundEnd]
    queries = []
    for _ in range(60):
        a, b = rng.choice(probes), rng.choice(probes)
        if SO._cmp(a, b) > 0 and rng.random() < 0.85:
            a, b = b, a
        if rng.random() < 0.1:
            a = P.UnboundStart
        lim = rng.choice([1, 2, 3, 7, 50, 10_000])
        queries.append((a, b, lim, rng.choice([ASC, DESC])))
    outs = _same_ranges(orc, dev, queries)
    assert sum(o[0] == "rows" and len(o[1]) > 0 for o in outs) > 5
    assert dev.range_stats["windows_accepted"] > 0


def test_get_ranges_quirk_snapshot(decoder):
    segs = SC.quirk_segments()
    orc, dev = _pair(segs, decoder)
    probes = [b"k%02d" % i for i in range(0, 62, 3)] + [b"k20", b"k25", b"k21"]
    md = P.bytes_to_metadata(segs[3][4])
    probes += [st.FirstKey for st in md.entries]
    queries = [(a, b, lim, d) for a in probes for b in probes for d in (ASC, DESC)
               for lim in (0, 2, 100)]
    outs = _same_ranges(orc, dev, queries)
    assert {"rows", "err", "panic"} <= {o[0] for o in outs}


def test_get_ranges_with_a_zstd_segment(decoder):
    from oracle import zstd_ref as Z
    segs, keys = SC.random_snapshot(7, nseg=3)
    rng = random.Random(8)
    zrows = [(k, b"" if rng.random() < 0.2 else b"z-" + k * 3) for k in keys[::2]]
    zseg, zn, zmeta = Z.zstd_segment(zrows, 700, 1024, level=3)
    segs.append(("0009-zstd", 0, zseg, zn, zmeta))
    orc, dev = _pair(segs, decoder)
    queries = [(a, b, lim, d) for a, b in ((keys[5], keys[-5]), (P.UnboundStart, keys[40]),
                                           (keys[100], P.UnboundEnd), (keys[30], keys[33]))
               for lim in (1, 4, 1000) for d in (ASC, DESC)]
    outs = _same_ranges(orc, dev, queries)
    assert any(o[0] == "rows" and any(v and v.startswith(b"z-") for _k, v in o[1]) for o in outs)
    assert not dev._rows["0009-zstd"].index_only and dev._rows[segs[0][0]].index_only


def test_resident_iter_paging(decoder):
    """snapshot_iter.go paging with resident=True, to io.EOF or the empty-page panic."""
    for seed in (11, 12, 13):
        segs, keys = SC.random_snapshot(seed, nseg=3)
        orc, dev = _pair(segs, decoder)
        for d, start in ((ASC, keys[3]), (DESC, keys[-4])):
            for buf in (3, 17):
                oi, di = orc.RowIter(start, d, buf), dev.RowIter(start, d, buf, resident=True)
                for _ in range(400):
                    a = _outcome(lambda: [oi.Next()])
                    b = _outcome(lambda: [di.Next()])
                    assert a == b
                    if a[0] != "rows":
                        break
                assert a[0] != "rows"
        assert not dev._segs  # no DeviceSegment (host copy) was built


def _write(rows):
    w = P.SegmentWriter(P.SegmentWriterOptions())
    for k, v in rows:
        w.WriteRow(k, v)
    n, meta = w.Close()
    return bytes(w.external), n, meta


def test_a_page_costs_the_page(decoder):
    """Three segments of 160 rows, limit 5 from the first key: the merge sees the windows,
    not the segments.  A run of L0 tombstones longer than the slack makes the one rerun."""
    limit = 5
    c = SN.window_size(limit)
    assert c == limit + 1 + 16
    keys = [b"key%05d" % i for i in range(480)]
    plain = [[(k, b"v%d-" % s + k) for k in keys[s::3]] for s in range(3)]
    segs = [("%04d" % (s + 1), 0 if s < 2 else 1) + _write(plain[s]) for s in range(3)]
    orc, dev = _pair(segs, decoder)
    q = (keys[0], P.UnboundEnd, limit, ASC)
    out = _same_ranges(orc, dev, [q])[0]
    assert out[0] == "rows" and len(out[1]) == limit
    st = dev.range_stats
    assert st["reruns"] == 0 and st["rows_merged"] <= 3 * c and st["windows_accepted"] == 1
    assert st["seeks"] == 3 and st["gather_calls"] == 1
    # the newest L0 segment opens with tombstones over the first c + 4 keys of the snapshot:
    # its window holds nothing else, and the loop rolls off its end (io.EOF, refused)
    tomb = [(k, b"") for k in keys[:c + 4]] + [r for r in plain[1] if r[0] > keys[c + 3]]
    segs[1] = ("0002", 0) + _write(tomb)
    orc, dev = _pair(segs, decoder)
    out = _same_ranges(orc, dev, [q])[0]
    assert out[0] == "rows" and len(out[1]) == limit
    st = dev.range_stats
    assert st["reruns"] == 1 and st["gather_calls"] == 2 and st["rows_merged"] > 3 * c
