"""Block-index cases shared by tests/test_index_host.py (okv_index.hpp on the CPU) and
tests/test_get_gpu.py (the floor search on the device): trees of first keys in
meta-block order, query keys, and what oracle/pyoracle.py's BlockIndex (google/btree
ReplaceOrInsert / DescendLessOrEqual) gives for them."""
from __future__ import annotations

from oracle import pyoracle as P


def _seq(n, width=4):
    return [b"k" + (7 * i + 3).to_bytes(width, "big") for i in range(n)]


def trees():
    """name -> first keys in meta-block order."""
    shared8 = b"prefix08"                       # 8 shared leading bytes
    shared9 = b"prefix09_"                      # 9
    shared16 = b"prefix16_________"[:16]        # 16
    t = {
        "one": [b"m"],
        "two": [b"b", b"a"],
        "three": [b"b", b"c", b"a"],
        "dups_last_wins": [b"a", b"b", b"a", b"c", b"b", b"b", b"d", b"a"],
        "empty_first_key": [b"", b"a", b"\x00", b"b"],
        "empty_dup": [b"x", b"", b"y", b""],
        "ab_family": [b"abc", b"ab", b"ab\x00", b"a", b"ab\x00\x00"],
        "short_and_zero": [b"ab", b"ab\x00", b"ab\x00\x00\x00\x00\x00\x00", b"ab\x00\x00\x00\x00\x00\x00\x00",
                           b"ab\x00\x00\x00\x00\x00\x01"],
        "prefix_ties": ([shared8 + s for s in (b"", b"a", b"b", b"ba", b"\xff")] +
                        [shared9 + s for s in (b"", b"\x00", b"0", b"00", b"1")] +
                        [shared16 + s for s in (b"", b"a", b"aa", b"ab", b"b", b"\xff\xff")]),
        "prefix_ties_dups": [shared9 + b"x", shared9 + b"y", shared9 + b"x", shared16 + b"q",
                             shared16 + b"q", shared8],
    }
    for n in (1, 2, 3, 63, 64, 65):
        ks = _seq(n)
        # meta-block order is not key order: rotate, and repeat one key (the last stays)
        t[f"n{n}"] = ks[n // 2:] + ks[:n // 2]
        t[f"n{n}_dup"] = ks + [ks[n // 3]]
    return t


def queries(first_keys):
    """Each first key, plus one byte, minus one byte; below the first entry; above the
    last; the ab family; and the prefix families cut and extended at 8, 9 and 16."""
    q = {b"", b"\x00", b"ab", b"ab\x00", b"abc", b"a", b"b", b"\xff" * 20, b"zzzz"}
    for k in set(first_keys):
        q |= {k, k + b"\x00", k + b"\x01", k + b"\xff"}
        if k:
            q.add(k[:-1])
            last = k[-1]
            if last > 0:
                q.add(k[:-1] + bytes([last - 1]))
            if last < 255:
                q.add(k[:-1] + bytes([last + 1]))
        for cut in (7, 8, 9, 15, 16, 17):
            if len(k) >= cut:
                q |= {k[:cut], k[:cut] + b"\x00", k[:cut] + b"\xff"}
    return sorted(q)


def oracle_tree(first_keys):
    """-> (file indices in tree order, the BlockIndex); Offset carries the file index."""
    ix = P.BlockIndex()
    for i, k in enumerate(first_keys):
        ix.replace_or_insert(P.BlockStat(FirstKey=k, Offset=i))
    return [st.Offset for st in ix.ascend()], ix


def oracle_floor(ix, key):
    """DescendLessOrEqual's first item as a file index, or -1."""
    le = ix.descend_le(key)
    return le[0].Offset if le else -1
