"""Blocks for the kernels that work from a block staged in LDS (okv_kernels.hpp, "a block
staged in LDS": the point kernel, the fused and small-gather kernels, the batched
GetRow's search), shared by the CPU test (tests/test_oracle.py: the two oracles agree and
the cases have the properties claimed) and the GPU tests (test_point_gpu.py,
test_decode_gpu.py, test_get_gpu.py).  Each case is (segment bytes, descriptors [n, 4]
uint64, probe keys), chosen for where a stage, a run-length walk or a masked compare can
go wrong."""
from __future__ import annotations

import functools

import numpy as np

# the device constants the cases are cut to (okv_kernels.hpp, okv_decode.hip, okv_get.hip)
FAST_ROWS = 1024        # kFastRows: rows of a staged block's row table
RCAP = 64               # kRCap: rows of a small block
STAGE = 65536           # kStage: the workgroup stage
SMALL_STAGE = 5 * 1024  # kSmallStage: the one-wave stage
FIND_KEY = 8192         # kFindKey: the longest okv_point_get probe
GET_CAPS = (8192, 65536)  # okv_get_search_kernel<kCap>
RUNS = (1, 2, 63, 64, 65, 128, 129)
BAD_LANES = (1, 63, 64)


def rec(k: bytes, v: bytes) -> bytes:
    return len(k).to_bytes(2, "little") + len(v).to_bytes(4, "little") + k + v


def small_need(offset: int, walk_end: int) -> int:
    """Stage bytes the one-wave form needs: lead-in, shift, the bytes, slack."""
    return 16 + (offset & 15) + walk_end + 32


def _layout(blocks, shifts=None, tail=0):
    """Bodies [(bytes, OriginalSize or None)] back to back, block b at an offset with
    offset & 15 == shifts[b] (default 0; the first block at 0 when its shift is 0), then
    `tail` bytes -> (seg, descs)."""
    seg, descs = bytearray(), []
    for b, (body, orig) in enumerate(blocks):
        sh = shifts[b] if shifts else 0
        seg += bytes((sh - len(seg)) & 15)
        descs.append((len(seg), len(body), len(body) if orig is None else orig, 0))
        seg += body
    seg += bytes(tail)
    return bytes(seg), np.array(descs, np.uint64).reshape(-1, 4)


def _run_block(n, k=b"rk", v=b"val"):
    """n identical records, a different one, the block's end."""
    return rec(k, v) * n + rec(b"other", b"z" * 9)


def _filled(rng, size, nrec):
    """nrec records that fill exactly `size` bytes (walk end == BlockSize == size)."""
    body = bytearray()
    vmax = max(1, size // nrec - 6 - 30)  # (so that the last record has room)
    for i in range(nrec - 1):
        kl, vl = int(rng.integers(1, 30)), int(rng.integers(0, vmax))
        body += rec(rng.integers(0, 256, kl, dtype=np.uint8).tobytes(),
                    rng.integers(0, 256, vl, dtype=np.uint8).tobytes())
    rest = size - len(body) - 6 - 4
    assert rest >= 0
    body += rec(b"last", rng.integers(0, 256, rest, dtype=np.uint8).tobytes())
    assert len(body) == size
    return bytes(body)


def _mixed_rows(rng, n):
    """n records of mixed non-zero key and value lengths, distinct keys."""
    body = bytearray()
    for i in range(n):
        kl, vl = 3 + int(rng.integers(0, 6)), 1 + int(rng.integers(0, 9))
        key = i.to_bytes(3, "big") + rng.integers(0, 256, kl - 3, dtype=np.uint8).tobytes()
        body += rec(key, rng.integers(0, 256, vl, dtype=np.uint8).tobytes())
    return bytes(body)


def _keys_of(body, every=1):
    """Keys of a well-formed body, every n-th."""
    keys, p = [], 0
    while p + 6 <= len(body):
        kl = int.from_bytes(body[p:p + 2], "little")
        vl = int.from_bytes(body[p + 2:p + 6], "little")
        keys.append(bytes(body[p + 6:p + 6 + kl]))
        p += 6 + kl + vl
    return keys[::every]


def bad_run_block(lane, kind):
    """A run of identical 11-byte records whose record `lane` (counted from the run's
    first: the lane that reads it in its round of 64) is bad -> (body, OriginalSize)."""
    good = rec(b"rk", b"val")
    body = bytearray(good * lane)
    if kind == "klen":      # key length past the block
        body += (0xffff).to_bytes(2, "little") + (3).to_bytes(4, "little") + b"rkval"
    elif kind == "vlen":    # value length past the block (also past 32 bits with the key's)
        body += (2).to_bytes(2, "little") + (0xffffffff).to_bytes(4, "little") + b"rkval"
    else:                   # "short": fewer than 6 bytes left, OriginalSize past them
        body += good[:5]
    return bytes(body), len(body) + 11


def key_block():
    """Rows for the masked compare: keys of every probe length, each after a row that
    differs from it in the last byte only and a row that is its strict prefix, and
    before a row it is a strict prefix of; two equal keys with different values."""
    rng = np.random.default_rng(77)
    body, probes = bytearray(), []
    for kl in (1, 3, 4, 5, 255, 256, FIND_KEY):
        key = bytes([kl & 255]) + rng.integers(1, 256, kl - 1, dtype=np.uint8).tobytes()
        near = key[:-1] + bytes([key[-1] ^ 1])
        body += rec(near, b"near%d" % kl) + rec(key[:-1], b"prefix%d" % kl)
        body += rec(key, b"hit%d" % kl) + rec(key + b"\x07", b"longer%d" % kl)
        probes += [key, near, key[:-1], key + b"\x07", key[:-1] + bytes([key[-1] ^ 0x80]),
                   key + b"\x00"]
    body += rec(b"dup", b"first") + rec(b"dup", b"second") + rec(b"", b"empty key")
    body += rec(b"dup", b"")
    probes += [b"dup", b"", b"absent", b"du", b"dupp", b"\x00"]
    return bytes(body), probes


@functools.lru_cache(maxsize=1)
def cases():
    """name -> (seg, descs, probe keys); built once, shared, not to be changed."""
    rng = np.random.default_rng(2024)
    c = {}
    # ---- walk ----
    c["runs"] = _layout([(_run_block(n), None) for n in RUNS]) + ([b"rk", b"other", b"r"],)
    same_len = [(3, 5), (5, 3), (4, 4), (0, 8)] * 5 + [(3, 5)] * 3
    body = b"".join(rec(bytes([65 + i % 26]) * kl, bytes([97 + i % 26]) * vl)
                    for i, (kl, vl) in enumerate(same_len))
    c["same_length_other_header"] = _layout([(body, None)]) + (_keys_of(body) + [b"AAAA"],)
    c["bad_in_run"] = _layout([bad_run_block(lane, kind) for lane in BAD_LANES
                               for kind in ("klen", "vlen", "short")]) + ([b"rk"],)
    run = _run_block(10)
    origs = [10 * 11, 3 * 11 + 1, 0, 2**63, 2**64 - 1, len(run) + 100]
    c["original_size"] = _layout([(run, o) for o in origs]) + ([b"rk", b"other"],)
    rows = [_mixed_rows(rng, n) for n in (FAST_ROWS - 1, FAST_ROWS, FAST_ROWS + 1)]
    c["fast_rows_edge"] = _layout([(r, None) for r in rows]) + \
        (_keys_of(rows[0], 97) + _keys_of(rows[2])[-2:] + [b"nope"],)
    # ---- staging ----
    # offsets & 15 in {0, 1, 15}, the first block at 0, the last ending at the segment's
    # last byte with seg_bytes % 16 != 0
    small = [_filled(rng, n, r) for n, r in ((333, 7), (1000, 7), (77, 2), (501, 7))]
    c["offsets"] = _layout([(s, None) for s in small], shifts=[0, 1, 15, 1]) + \
        (_keys_of(small[3]) + [b"last"],)
    # the one-wave stage filled exactly, and one byte more (the HBM source), at shift 0
    # and 15
    full = [(SMALL_STAGE - 48, 0), (SMALL_STAGE - 47, 0), (SMALL_STAGE - 63, 15),
            (SMALL_STAGE - 62, 15)]
    c["small_stage_edge"] = _layout([(_filled(rng, n, 9), None) for n, _ in full],
                                    shifts=[s for _, s in full], tail=3) + ([b"last", b"l"],)
    # the workgroup stage's last piece: a 64 KiB block at offset & 15 == 15
    big = _filled(rng, STAGE, 300)
    c["stage_last_piece"] = _layout([(big, None)], shifts=[15]) + \
        (_keys_of(big, 50) + [b"last"],)
    # the two search instantiations
    c["get_caps"] = _layout([(_filled(rng, GET_CAPS[0], 40), None),
                             (_filled(rng, GET_CAPS[0] + 1, 40), None)]) + ([b"last", b"x"],)
    # ---- key compare ----
    body, probes = key_block()
    c["keys"] = _layout([(body, None)], shifts=[3]) + (probes,)
    return c


WALK = ("runs", "same_length_other_header", "bad_in_run", "original_size", "fast_rows_edge")
STAGING = ("offsets", "small_stage_edge", "stage_last_piece", "get_caps")
KEYS = ("keys",)
