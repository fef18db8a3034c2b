"""The CPU model of the device zstd encoder's parse (tests/zenc_model.py), without a GPU:
over every row set the GPU tests encode, the model's frame inflates with libzstd to the
block, every frame is within the interface bound, and each parse fixture is the shape it
claims to be -- asserted from the model's census alone, so that the GPU test, which holds
the device's frames against the model byte for byte, is known to walk those paths.

zenc_main is built here with AddressSanitizer and UBSan and run as a plain program."""
from __future__ import annotations

import pytest

from oracle import zstd_ref as Z
from tests import zenc_cases as ZC
from tests import zenc_model as M

UNIT = M.UNIT
SEEN = {"ll": set(), "ml": set(), "of": set(), "lit_form": set(), "nseq_form": set(),
        "block": set()}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return M.build_zenc_main(str(tmp_path_factory.mktemp("zenc") / "zenc_main"), sanitize=True)


DONE = {}


def _units(exe, rows, T, name):
    """Model of every block of the rows: round trip, bound, census gathered; the units
    (computed once per row set and threshold)."""
    if (name, T) not in DONE:
        DONE[name, T] = _model_units(exe, rows, T)
    return DONE[name, T]


def _model_units(exe, rows, T):
    raws = ZC.blocks_of(rows, T)
    units = []
    for raw, (frame, us) in zip(raws, M.model_frames(raws, exe)):
        assert Z.decompress(frame, len(raw)) == raw
        assert len(frame) <= len(raw) + 3 * -(-len(raw) // UNIT) + 18
        assert [u.n for u in us] == [min(UNIT, len(raw) - i) for i in range(0, len(raw), UNIT)]
        for u in us:
            c = u.census
            assert sum(c["seq_per_quarter"]) == len(u.seqs)
            assert sum(ll + ml for ll, ml, _ in u.seqs) + u.tail == u.n
            assert c["block"] == (2 if u.seqs and c["csz_minus_n"] < 0 else 0)
            for k in ("ll", "ml", "of"):
                SEEN[k] |= c[k]
            for k in ("lit_form", "nseq_form", "block"):
                SEEN[k].add(c[k])
        units += us
    return units


@pytest.mark.parametrize("T,D", ZC.CONFIGS)
def test_corpus_round_trip_and_bound(exe, T, D):
    for name, rows in ZC.corpus(T):
        _units(exe, rows, T, name)


@pytest.mark.parametrize("name,T,D", [(n, T, D) for n, T, D, _ in ZC.writer_cases()])
def test_writer_cases_round_trip_and_bound(exe, name, T, D):
    rows = {n: r for n, _T, _D, r in ZC.writer_cases()}[name]
    units = _units(exe, rows, T, name.rsplit('_D', 1)[0])
    if name.startswith("long_first_keys"):
        raws = ZC.blocks_of(rows, T)
        assert len(raws) == len(rows) >= 600 and max(len(k) for k, _ in rows) == 65535
        assert sum(300 <= len(k) <= 2000 for k, _ in rows) >= 600
        g = ZC.meta_group_bytes([k for k, _ in rows])
        assert g[0] > ZC.META_IMAGE and g[1] + 30 <= ZC.META_IMAGE and g[2] > ZC.META_IMAGE
    if T == 70000:
        assert max(len(r) for r in ZC.blocks_of(rows, T)) > 2 * UNIT and len(units) >= 9


@pytest.mark.parametrize("T,D", ZC.CONFIGS)
@pytest.mark.parametrize("name", [n for n, _, ok in ZC.parse_fixtures() if ok])
def test_parse_fixture_is_what_it_claims(exe, T, D, name):
    """The fixture's condition (tests/zenc_cases.py, the *_ok function beside each fixture)
    holds for the blocks the rows are cut into at this threshold."""
    rows, ok = {n: (r, f) for n, r, f in ZC.parse_fixtures()}[name]
    ok(_units(exe, rows, T, name))


def test_code_sweep_reaches_every_code(exe):
    """Over the corpus every literal-length, match-length and offset code the parse can
    reach is used, and no other.  What it can reach, for a unit of 32 768 bytes in quarters
    of 8 192:

    * offset: a distance is 1 .. 32 764 (a match starts at n - 4 at the latest, its source at
      0), coded as distance + 3 = 4 .. 32 767: codes 2 .. 14.
    * match length: 4 .. 8 192 (a match lies inside one quarter); the code of 8 192 is 48
      (4 099 .. 8 194): codes 1 .. 48 (code 0 is length 3).
    * literal length: 0 .. 32 764 (three quarters without a sequence and the last one up to
      its last legal start); the code of 32 764 is 33 (16 384 .. 32 767): codes 0 .. 33.

    Also: both block types, the three literals-header forms and the 1- and 2-byte
    Number_of_Sequences forms."""
    for T, _D in ZC.CONFIGS:
        for name, rows in ZC.corpus(T):
            _units(exe, rows, T, name)
    for k in ("ll", "ml", "of"):
        assert SEEN[k] == ZC.REACHABLE[k], (k, sorted(SEEN[k] ^ ZC.REACHABLE[k]))
    assert M.code(M.LL, 32764) == 33 and M.code(M.ML, 8192) == 48
    assert SEEN["block"] == {0, 2}
    assert SEEN["lit_form"] - {None} == {1, 2, 3} and SEEN["nseq_form"] - {None} == {1, 2}
