"""Snapshot GetRows with OKV_F_GET_ZSTD: a zstd candidate answers, moves on
or ends the key like any other.  The expectation is tests/test_snap_get_gpu.py's Env.expect
restated with the per-candidate outcome taken from pyoracle.read_block (which reports a
rejected frame set as status 6, where pyoracle's GetRow says ErrNoRows) plus the row loop."""
from __future__ import annotations

import functools

import pytest

from objectkv_amd import _lib, snap as S
from oracle import pyoracle as P
from oracle import snapshot_oracle as SO
from oracle import zstd_ref as Z
from tests.test_snap_get_gpu import (DELETED, FALLBACK, FOUND, NO_ROWS, NONE32, SEG_ERROR, Env,
                                     _read_status, _returned, _seg, _zstd_seg)

pytestmark = pytest.mark.gpu


class ZEnv(Env):
    def candidate(self, rec, key, blocks):
        """One candidate's GetRow under the flag -> None (ErrNoRows) or
        (state, blk_status, value, entry)."""
        rd = self.readers[rec.ID]
        md = rd._md()
        if md.BloomFilter is not None and not md._bloom.test(P._b(key)):
            return None
        floor = md.BlockIndex.descend_le(key)
        if not floor:
            return None
        st = floor[0]
        d = st.desc()
        zstd = md.compression == P.COMP_ZSTD
        rs = _read_status(d, len(rd.data))
        if rs == _lib.BLK_OK and zstd and d[3] > d[1]:
            rs = _lib.BLK_PANIC
        if rs != _lib.BLK_OK:
            return SEG_ERROR, rs, None
        if not zstd and st.BlockSize > 65536:
            return FALLBACK, 0, None
        blocks.add((rec.ID, st.Offset))
        if zstd:
            raw = Z.decompress(rd.data[d[0]:d[0] + d[3]], d[2])
            if raw is not None and len(raw) > _lib.GET_INFLATED_MAX:
                return FALLBACK, 0, None
        bst, rows = P.read_block(rd.data, d, md.compression)
        if bst:
            return SEG_ERROR, bst, None
        for r in rows or []:
            if P._b(r.Key) == P._b(key):
                if not P._b(r.Value) and rec.Level == 0:
                    return DELETED, 0, None
                return FOUND, 0, r.Value
        return None

    def expect(self, key, blocks):
        """(state, segment ID, blk_status, value) and the candidate count; every candidate
        is probed, so `blocks` collects every one's floor block."""
        cands = sorted(self.orc.getPossibleSegmentsForKey(key),
                       key=functools.cmp_to_key(SO._getrow_cmp))
        answer = None
        for rec in cands:
            got = self.candidate(rec, key, blocks)
            if got is not None and answer is None:
                answer = (got[0], rec.ID, got[1], got[2])
        return answer or (NO_ROWS, None, 0, None), len(cands)


def _check(env, keys, reader=True):
    res = S.snap_get_rows(env.dec, env.snap, keys, zstd=True)
    blocks, pairs, tot, pos = set(), 0, [0, 0, 0, 0, 0], 0
    for i, k in enumerate(keys):
        (st, sid, bst, val), nc = env.expect(k, blocks)
        pairs += nc
        got_id = None if int(res.seg[i]) == NONE32 else env.snap.ids[int(res.seg[i])]
        assert (int(res.state[i]), got_id, int(res.blk_status[i])) == (st, sid, bst), k
        tot[st] += 1
        if st == FOUND:
            v = P._b(val)
            assert res.value(i) == val and int(res.val_len[i]) == len(v), k
            assert int(res.val_pos[i]) == pos
            pos += (len(v) + 15) // 16 * 16
            rd = env.readers[sid]
            off = int(res.val_off[i])
            if rd._md().compression == P.COMP_ZSTD:  # inside the inflated block entry[i]
                d = rd._md().entries[int(res.entry[i])].desc()
                raw = Z.decompress(rd.data[d[0]:d[0] + d[3]], d[2])
                assert raw[off:off + len(v)] == v, k
            else:
                assert env.data[sid][0][off:off + len(v)] == v, k
        else:
            assert int(res.val_len[i]) == 0 and int(res.val_off[i]) == 0
    assert (res.n_found, res.n_deleted, res.n_fallback, res.val_bytes) == \
        (tot[FOUND], tot[DELETED], tot[FALLBACK], pos)
    assert res.blocks_searched == len(blocks) and res.pairs_probed == pairs
    if reader:  # snapshot.Reader.GetRows == the per-key outcomes
        got = env.dev.GetRows(keys)
        for i, (k, g) in enumerate(zip(keys, got)):
            st = int(res.state[i])
            if st == FOUND:
                assert _returned(g) == ("value", res.value(i)), k
            elif st in (NO_ROWS, DELETED):
                assert _returned(g) == ("err", P.ErrNoRows), k
            elif st == SEG_ERROR:
                want = {_lib.BLK_PANIC: ("panic",), _lib.BLK_ZSTD_ERROR: ("err", "ZstdError"),
                        _lib.BLK_EOF: ("err", "EOF")}.get(int(res.blk_status[i]))
                assert _returned(g) == (want or ("err", "ErrUnexpectedBytesRead")), k
    return res


def test_zstd_candidate_answers(decoder):
    """The two scenarios of test_fallback's zstd case with the flag: nothing falls back."""
    rows = [(b"k%03d" % i, b"v%03d" % i * 3) for i in range(60)]
    part = [(k, b"new-" + v) for k, v in rows if k not in (b"k030", b"k031")] + \
        [(b"k0305", b"keeps k030 inside the range")]
    part.sort()
    older = _zstd_seg("1", 1, rows)
    env = ZEnv(decoder, [_seg("2", 0, part), older])
    res = _check(env, [b"k030", b"k010", b"k031", b"k0305", b"nope"])
    assert [int(s) for s in res.state] == [FOUND, FOUND, FOUND, FOUND, NO_ROWS]
    assert env.snap.ids[int(res.seg[0])] == "1" and res.n_fallback == 0
    assert res.value(0) == dict(rows)[b"k030"] and res.value(1) == b"new-" + dict(rows)[b"k010"]
    assert decoder.last_path() == _lib.PATH_SNAP_GET | _lib.PATH_ZSTD
    no_flag = S.snap_get_rows(decoder, env.snap, [b"k030", b"k010"])
    assert [int(s) for s in no_flag.state] == [FALLBACK, FOUND]
    env.close()
    env = ZEnv(decoder, [older, _seg("0", 2, rows)])
    res = _check(env, [b"k030", b"k010"])
    assert [int(s) for s in res.state] == [FOUND, FOUND] and res.n_fallback == 0
    assert {env.snap.ids[int(s)] for s in res.seg} == {"1"}
    env.close()


def _zseg(sid, lvl, rows, frame_fn=None):
    data, n, meta = Z.zstd_segment(rows, 3584, 4096, frame_fn=frame_fn)
    return (sid, lvl, data, n, meta)


def test_mixed_kinds(decoder):
    """Six overlapping L0 / L1 segments, alternately zstd and uncompressed: tombstones in a
    zstd L0 segment, shadowing across kinds, one staging per (segment, block)."""
    def val(s, i):
        return b"s%d-" % s + b"%05d" % i * (1 + (i + s) % 40)
    segs = []
    for s in range(6):
        lvl = 0 if s >= 3 else 1
        rows = [(b"k%04d" % i, b"" if (lvl == 0 and i % 11 == s) else val(s, i))
                for i in range(s * 40, s * 40 + 400, 1 + s % 3)]
        segs.append((_zseg if s % 2 else _seg)("%d" % s, lvl, rows))
    env = ZEnv(decoder, segs)
    keys = [b"k%04d" % i for i in range(90, 560)] + [b"k0100x", b"", b"zzz"]
    res = _check(env, keys)
    states = {int(s) for s in res.state}
    assert {FOUND, NO_ROWS, DELETED} <= states and res.n_fallback == 0
    kinds = {(int(s), env.readers[env.snap.ids[int(g)]]._md().compression)
             for s, g in zip(res.state, res.seg) if int(g) != NONE32}
    assert {(FOUND, 0), (FOUND, 1), (DELETED, 1)} <= kinds
    env.close()


def test_corrupt_frame_and_cap(decoder):
    """A corrupt frame in the newer zstd candidate ends the key (SEG_ERROR, status 6);
    behind a newer answer it is hidden.  A candidate over the cap is still FALLBACK."""
    rows = [(b"k%03d" % i, b"value %03d " % i * 20) for i in range(120)]
    bad = _zseg("5", 0, rows, frame_fn=lambda raw, i: Z.compress(raw)[:-3] if i == 2
                else Z.compress(raw))
    md = P.bytes_to_metadata(bad[4])
    lo, hi = P._b(md.entries[2].FirstKey), P._b(md.entries[3].FirstKey)
    in_bad = [k for k, _ in rows if lo <= k < hi]
    assert in_bad
    env = ZEnv(decoder, [bad, _seg("1", 1, rows)])
    res = _check(env, in_bad[:3] + [rows[0][0], b"nope"])
    assert [(int(s), int(b)) for s, b in zip(res.state, res.blk_status)][:3] == \
        [(SEG_ERROR, _lib.BLK_ZSTD_ERROR)] * 3
    assert int(res.state[3]) == FOUND and env.snap.ids[int(res.seg[3])] == "5"
    env.close()
    env = ZEnv(decoder, [_seg("9", 0, [(k, b"newer") for k, _ in rows]), bad])
    res = _check(env, in_bad[:3])
    assert all(int(s) == FOUND and res.value(i) == b"newer" for i, s in enumerate(res.state))
    env.close()
    huge = Z.zstd_segment([(b"a", bytes((1 << 24) - 6)), (b"b", b"x")], 1 << 26, 4096)
    env = ZEnv(decoder, [("7", 0) + huge, _seg("1", 1, [(b"a", b"old"), (b"b", b"old")])])
    res = _check(env, [b"a", b"b", b"c"], reader=False)
    assert [int(s) for s in res.state] == [FALLBACK, FALLBACK, NO_ROWS] and res.n_fallback == 2
    env.close()
