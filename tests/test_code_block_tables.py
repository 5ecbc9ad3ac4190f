"""CPU: the tables every code-block size depends on, for all 188 sizes, against
the reference's own tables (tests/golden/make_golden_cb_tables.py ->
golden_cb_tables.json): the QPP rows, the interleaver sizes and
get_segmentation_info on a boundary list of transport-block sizes.  The
library's host index maps (lte_qpp_perm, lte_subblock_perm,
lte_rate_dematch_map: no GPU needed) and the drop-in's segmentation are
checked against the fixture and, where the fixture has no entry, against the
oracle, which is itself checked against the fixture here.  All exact."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import ROOT

FIX = os.path.join(ROOT, 'tests', 'golden', 'golden_cb_tables.json')
TAB = json.load(open(FIX))
QPP_ROWS = [tuple(r) for r in TAB['qpp']]
SIZES = [r[0] for r in QPP_ROWS]
B_MAX = 6144 * 13
# (E, rv) of the rate-matching shapes: full buffer, heavy puncturing, puncturing
# that ends inside the parity part, repetition (E > N_cb = 3K + 18)
RM_SHAPES = [(lambda K: 3 * K + 12, 0), (lambda K: K + 17, 2), (lambda K: 2 * K + 5, 1), (lambda K: 4 * K, 3)]


@pytest.fixture(scope='module')
def cc():
    from lte_phy import channel_coding
    return channel_coding


def test_fixture_is_the_recorded_one():
    man = json.load(open(FIX.replace('.json', '_manifest.json')))
    assert hashlib.sha256(open(FIX, 'rb').read()).hexdigest() == man['sha256']
    assert {k: len(v) for k, v in TAB.items()} == man['rows']
    assert len(QPP_ROWS) == 188 and SIZES == sorted(set(SIZES)) == TAB['sizes']


def test_size_tables_equal_the_reference(cc, oracle):
    assert cc.TURBO_INTERLEAVER_SIZES == TAB['sizes']
    assert oracle.TURBO_SIZES == TAB['sizes']
    assert [(K,) + tuple(oracle.QPP[K]) for K in sorted(oracle.QPP)] == QPP_ROWS


def test_qpp_perm_every_size(cc, oracle):
    """lte_qpp_perm(K) (QPP_TAB of lte_capi.hip, the table the encoder and the
    decoders walk) == (f1 i + f2 i^2) mod K from the reference's row, and is a
    permutation, for every K; an illegal K is refused."""
    for K, f1, f2 in QPP_ROWS:
        i = np.arange(K, dtype=np.int64)
        want = (f1 * i + f2 * i * i) % K
        got = cc._qpp(K)
        assert np.array_equal(got, want), K
        assert np.array_equal(np.sort(got), i), K
        assert np.array_equal(oracle.qpp_perm(K), want), K
    for K in (39, 41, 520, 1040, 2080, 6145):
        with pytest.raises(ValueError, match=f'Invalid interleaver size K={K}'):
            cc._qpp(K)


def test_segmentation_info_boundaries(cc, oracle):
    """get_segmentation_info at K - 1 / K / K + 1 of every size, 6144 / 6145
    and the first, last and a two-size B of C = 2..13 blocks: the drop-in and
    the oracle's plan equal the reference's answer."""
    seen_c = set()
    for B, n, sizes, total in TAB['seg_info']:
        want = {'num_blocks': n, 'block_sizes': sizes, 'total_coded_bits': total}
        assert cc.get_segmentation_info(B) == want, B
        plan = oracle.segmentation_plan(B)
        assert [p[0] for p in plan] == sizes and sum(3 * p[0] + 12 for p in plan) == total, B
        seen_c.add(n)
    assert seen_c == set(range(1, 14))
    bs = {r[0] for r in TAB['seg_info']}
    assert all({K - 1, K, K + 1} <= bs | {0} for K in SIZES) and {6144, 6145, 6120 * 13} <= bs


def test_segmentation_every_size(cc, oracle):
    """Every transport-block size with CRC from 25 (one payload bit) to 13 full
    blocks: the drop-in's block sizes, information bits and filler per block
    equal the oracle's plan (whose boundary values equal the reference above),
    and the plan is consistent (fillers only where the reference puts them,
    every bit placed once)."""
    for B in range(25, B_MAX + 1):
        plan = oracle.segmentation_plan(B)
        sizes = [p[0] for p in plan]
        assert cc.segmentation_sizes(B) == sizes, B
        info = cc._bits_per_block(B, sizes) if B > 6144 else [B]
        assert info == [p[2] for p in plan], B
        crc = 24 if B > 6144 else 0
        assert [K - crc - n for K, n in zip(sizes, info)] == [p[1] for p in plan], B
        assert sum(info) == B and min(p[1] for p in plan) >= 0 and [p[3] for p in plan] == \
            list(np.cumsum([0] + info[:-1])), B


def test_single_block_metadata_every_size(cc, oracle):
    """segment_code_blocks for B = K - 1, K and the smallest B of each K (no
    device call for one block): filler count and positions, fillers first."""
    prev = 0
    for K in SIZES:
        for B in sorted({prev + 1, K - 1, K} - {0}):
            tb = np.ones(B, dtype=np.uint8)
            blocks, md = cc.segment_code_blocks(tb)
            (Ko, F, info, off, crc), = oracle.segmentation_plan(B)
            assert (Ko, info, off, crc) == (K, B, 0, False)
            assert md == {'num_blocks': 1, 'block_sizes': [K], 'num_filler_bits': F,
                          'filler_positions': list(range(F)), 'filler_per_block': [F], 'original_size': B,
                          'segmented': False}, B
            assert len(blocks) == 1 and not blocks[0][:F].any() and blocks[0][F:].all() and len(blocks[0]) == K
            assert np.array_equal(cc.desegment_code_blocks(blocks, md), tb)
        prev = K


def test_subblock_perm_every_size(cc, oracle):
    """lte_subblock_perm for the two stream lengths of every K (K + 6 with the
    tail split of d0, K + 3 for the parity streams)."""
    for K in SIZES:
        for n in (K + 3, K + 6):
            got = cc._sbi(n)
            assert np.array_equal(got, oracle.subblock_perm(n)), (K, n)
            assert np.array_equal(np.sort(got), np.arange(n)), (K, n)


def test_rate_dematch_map_every_size(oracle):
    """lte_rate_dematch_map (the table k_dematch / k_dematch_zn and the TX's
    rate matching are built from) for every K and four (E, rv) shapes: the
    values 1..E pushed through the map equal oracle.rate_dematch of them
    (1-based, so that the position fed by index 0 differs from a punctured
    one).  E = 4K > N_cb repeats: the map refuses it (the device sums repeats),
    and its map of one full buffer, wrapped and summed, gives the same."""
    from lte_phy import _capi as C
    for K in SIZES:
        Ncb = 3 * K + 18
        for fE, rv in RM_SHAPES:
            E = fE(K)
            x = np.arange(1, E + 1, dtype=np.float64)
            want = oracle.rate_dematch(x, K, rv)
            if E > Ncb:
                with pytest.raises(NotImplementedError, match='repeats'):
                    C.rate_dematch_map(K, E, rv)
                assert E < 2 * Ncb
                src = C.rate_dematch_map(K, Ncb, rv)
                got = np.where(src >= 0, src + 1.0, 0.0)
                again = (src >= 0) & (src + Ncb < E)
                got[again] += src[again] + Ncb + 1.0
            else:
                src = C.rate_dematch_map(K, E, rv)
                got = np.where(src >= 0, x[np.maximum(src, 0)], 0.0)
            assert src.shape == (3 * K + 12,) and src.max() < min(E, Ncb)
            assert np.array_equal(got, want), (K, E, rv)
            fed = src[src >= 0]
            assert len(np.unique(fed)) == len(fed), (K, E, rv)     # no received value used twice


def test_rate_match_is_the_inverse_every_size(cc, oracle):
    """The drop-in's rate_match_turbo (the dematch map inverted) == the
    oracle's rate matching for every K and the same shapes."""
    rs = np.random.RandomState(7)
    for K in SIZES:
        enc = rs.randint(0, 2, 3 * K + 12).astype(np.uint8)
        for fE, rv in RM_SHAPES:
            assert np.array_equal(cc.rate_match_turbo(enc, fE(K), K, rv), oracle.rate_match(enc, fE(K), K, rv)), \
                (K, fE(K), rv)
