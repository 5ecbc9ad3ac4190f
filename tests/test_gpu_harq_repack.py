"""GPU: opt-in re-packing of the unacknowledged frames of a HARQ process
(lte_plan_set_harq_repack) against the same process with the setting off on a
fresh plan and against the model of tests/harq_repack_model.py.

Numerology A of tests/test_gpu_harq.py (1.25 MHz, QPSK, AWGN), 2 iterations,
rv order (0, 2, 3, 1), max_tx = 4; TB 435 (one code block, 3K + 12 bits per
transmission) and TB 6121 in 8602 bits (two blocks, E = 4300 / 4302).  Frames
get per-frame SNRs, so the group classes are there by construction:

  HI_DB  acknowledged in the first round that can pass (round 0; round 1 at
         the punctured budget, whose rv 0 window cannot pass alone)
  LO_DB  never acknowledged
  ladder SNRs over the range in which tests/test_gpu_harq.py's LADDER puts the
         acknowledgements after 2, 3 and 4 transmissions

A group of HI frames is finished, one of LO frames full, and one of HI, LO and
ladder frames (in a shuffled lane order) mixed with a known number of active
lanes: between its LO frames and its LO + ladder frames.  The classes are
asserted from the run's own tx_used.  Everything is exact."""
import gc

import numpy as np
import pytest

import harq_model as M
import harq_repack_model as RM

pytestmark = pytest.mark.gpu

ITERS = 2
RV = (0, 2, 3, 1)
MAX_TX = 4
HI_DB, LO_DB = 12.0, -20.0
SWITCHES = ('LTE_TXCH_FUSE', 'LTE_RX_FUSE', 'LTE_TX_FRAME', 'LTE_RX_WAVE', 'LTE_TX_WAVE', 'LTE_DEMAP_IN_DEMATCH',
            'LTE_TXW_STAGE', 'LTE_TX_STAGE', 'LTE_HARQ_SKIP')
KEYS = ('counts', 'frame_errors', 'crc_ok', 'tx_used')
# (TB, coded_bits) -> the ladder's SNR range and the transmissions a HI frame takes
TBS = {435: dict(G=0, ladder=(0.0, 3.0), hi_tx=1), 6121: dict(G=8602, ladder=(3.0, 7.0), hi_tx=2)}
FIN, FULL = ('fin',), ('full',)


def mix(hi, ladder, lo, valid=64):
    assert hi + ladder + lo == valid
    return ('mix', hi, ladder, lo)


# name -> TB, the plan's max_frames and the groups.  The active lanes of a mixed
# group lie in [lo, lo + ladder], which fixes M, P and the rule's verdict:
#   partly      M = 3, A in [28, 48]: P = 1, cap = 2 -- packs, the packed group partly filled
#   two_packed  M = 3, A in [102, 120]: P = 2 < 3, cap = 2 -- packs, the second packed group partly filled
#   in_place    M = 2, A in [92, 100]: P = 2 = M (cap = 2) -- the rule says in place
#   over_cap    M = 3, A in [102, 120]: P = 2 > cap = 1 -- over capacity, in place
#   two_block   M = 3, A in [20, 44] from round 2 on: P = 1, cap = 2 -- packs, two code blocks of unequal E
CASES = {
    'partly': (435, 263, [FIN, mix(44, 8, 12), mix(40, 10, 14), FULL, mix(3, 2, 2, 7)]),
    'two_packed': (435, 320, [FIN, mix(24, 6, 34), mix(24, 6, 34), mix(24, 6, 34), FULL]),
    'in_place': (435, 320, [FIN, mix(14, 4, 46), mix(14, 4, 46)]),
    'over_cap': (435, 256, [FIN, mix(24, 6, 34), mix(24, 6, 34), mix(24, 6, 34)]),
    'two_block': (6121, 320, [mix(46, 10, 8), mix(44, 12, 8), mix(3, 2, 2, 7)]),
}
PACKS = {'partly': 1, 'two_packed': 2, 'two_block': 1}      # the P of the rounds that must pack


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


def clear_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def inputs(name):
    """(bits, per-frame SNRs) of a case; the lane order inside a mixed group is shuffled."""
    tb, _, groups = CASES[name]
    rs = np.random.RandomState(len(name) + tb)
    lad = TBS[tb]['ladder']
    snrs = []
    for g in groups:
        if g[0] == 'fin':
            snrs.append(np.full(64, HI_DB))
        elif g[0] == 'full':
            snrs.append(np.full(64, LO_DB))
        else:
            _, hi, ladder, lo = g
            v = np.concatenate([np.full(hi, HI_DB), np.linspace(lad[0], lad[1], ladder), np.full(lo, LO_DB)])
            snrs.append(v[rs.permutation(len(v))])
    snrs = np.concatenate(snrs)
    bits = rs.randint(0, 2, (len(snrs), tb)).astype(np.uint8)
    return bits, snrs


def make_plan(C, tb, prec, max_frames, repack, scale=None):
    import lte_phy
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn',
                                precision=prec)
    if scale is not None:
        sim.turbo_scale = scale
    return sim._plan(C.CHAIN_CODED, 0, tb, max_frames=max_frames, iters=ITERS,
                     harq=dict(max_tx=MAX_TX, rv_seq=RV, coded_bits=TBS[tb]['G']), harq_repack=repack)


def one_round(plan, t, snrs, capture=('bits_rx',), **kw):
    """Round t of the process, its results copied."""
    plan.harq_round(t)
    r = plan.run(snrs, capture=capture, **kw)
    d = {k: np.array(r[k]) for k in KEYS + tuple(capture)}
    d.update(path=dict(r.path), harq_info=r['harq_info'], info=r.get('harq_repack_info'))
    return d


def rounds(plan, snrs, capture=('bits_rx',), **kw):
    """The process's four rounds, each round's results copied."""
    return [one_round(plan, t, snrs, capture, **kw) for t in range(MAX_TX)]


def both(C, tb, prec, max_frames, snrs, capture=('bits_rx',), scale=None, **kw):
    """(setting off, setting on), each on a fresh plan."""
    from lte_phy import engine
    engine.clear_cache()
    off_plan = make_plan(C, tb, prec, max_frames, False, scale)
    on_plan = make_plan(C, tb, prec, max_frames, True, scale)
    assert off_plan is not on_plan and not off_plan.harq_repack and on_plan.harq_repack
    assert C.load().lte_plan_harq_repack(on_plan.h) == 1 and C.load().lte_plan_harq_repack(off_plan.h) == 0
    off, on = rounds(off_plan, snrs, capture, **kw), rounds(on_plan, snrs, capture, **kw)
    return off, on, on_plan


def check_on_against_off(C, off, on, cap, tag, skip_aware=True, identical=False):
    """What the issue fixes for every round: the latched results, harq_info and
    the path's harq field equal the process with the setting off; bits_rx of
    every frame unacknowledged before the round equals; a frame acknowledged in
    round s keeps round s's bits_rx in every later round that packs; the
    reported M, A, P, state and waves are the rule's on the previous round's
    crc_ok.  identical: bits_rx equal throughout and no round packs."""
    B = len(on[0]['crc_ok'])
    states = []
    for t in range(MAX_TX):
        a, b = off[t], on[t]
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), (tag, t, k)
        assert a['harq_info'] == b['harq_info'], (tag, t)
        assert a['path']['harq'] == b['path']['harq'] and 'harq_repack' not in a['path'], (tag, t)
        assert b['path']['harq_repack'] == '1' and {k: v for k, v in b['path'].items() if k != 'harq_repack'} == \
            a['path'], (tag, t)
        assert a['info'] is None
        info = b['info']
        assert info['on'] and info['cap'] == cap, (tag, t, info)
        if t == 0:
            assert (info['state'], info['M'], info['A'], info['P']) == ('none', 0, 0, 0), (tag, info)
            assert info['waves'] == -(-B // 64)
            states.append('none')
            continue
        prev = on[t - 1]['crc_ok']
        want = C.harq_repack_rule(prev, cap)
        assert want == RM.rule(prev, cap)
        assert (info['M'], info['A'], info['P']) == (want['M'], want['A'], want['P']), (tag, t, info, want)
        packs = want['pack'] and skip_aware
        assert info['state'] == ('packed' if packs else 'in_place'), (tag, t, info, want)
        assert info['waves'] == (want['waves_on'] if skip_aware else -(-B // 64)), (tag, t, info, want)
        states.append(info['state'])
        active = prev == 0
        assert np.array_equal(a['bits_rx'][active], b['bits_rx'][active]), (tag, t)
        if packs:
            # acknowledged in round s, every round since packed: the decisions of round s stay
            for s in (s for s in range(t) if all(st == 'packed' for st in states[s + 1:t])):
                at_s = (on[s]['crc_ok'] != 0) & ((on[s - 1]['crc_ok'] == 0) if s else True)
                assert np.array_equal(b['bits_rx'][at_s], on[s]['bits_rx'][at_s]), (tag, t, s)
        if identical:
            assert np.array_equal(a['bits_rx'], b['bits_rx']), (tag, t)
    if identical:
        assert 'packed' not in states, (tag, states)
    return states


_RUNS = {}


def case_runs(C, O, name, prec):
    """One case's three processes, computed once: setting off, setting on, the model on the on-run's own LLRs."""
    if (name, prec) not in _RUNS:
        tb, max_frames, _ = CASES[name]
        bits, snrs = inputs(name)
        off, on, plan = both(C, tb, prec, max_frames, snrs, capture=('bits_rx', 'llr'), seed=tb, bits=bits)
        num = O.Numerology(bandwidth=1.25, modulation='QPSK')
        Ks, Es = M.split(O, tb, num.bps, TBS[tb]['G'])
        assert plan.harq_info()['E'] == Es
        cap = RM.pack_cap(-(-max_frames // 64))
        proc = RM.Process(O, O.segmentation_plan(tb + 24), Es, RV, bits, ITERS, f32=(prec == 'f32'), cap=cap)
        model = []
        for t in range(MAX_TX):
            llr = [M.llr_coded_order(on[t]['llr'][b], num, sum(Es)) for b in range(len(snrs))]
            m = proc.round(t, llr)
            m['counts'] = proc.counts()
            model.append(m)
        _RUNS[name, prec] = (off, on, model, cap)
    return _RUNS[name, prec]


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('name', list(CASES))
def test_rounds_equal_the_setting_off_and_the_model(C, oracle, monkeypatch, name, prec):
    clear_switches(monkeypatch)
    tb, max_frames, groups = CASES[name]
    off, on, model, cap = case_runs(C, oracle, name, prec)
    tag = (name, prec)
    states = check_on_against_off(C, off, on, cap, tag, identical=name in ('in_place', 'over_cap'))
    for t in range(MAX_TX):
        m = model[t]
        for k in KEYS + ('bits_rx',):
            bad = np.flatnonzero(np.any(np.atleast_2d(on[t][k].T != m[k].T), axis=0))
            assert np.array_equal(on[t][k], m[k]), (tag, t, k, bad)
        assert on[t]['harq_info']['skipped'] == m['skipped'] and on[t]['info']['state'] == m['state'], (tag, t)
        assert on[t]['path']['dematch'] == 'llr' and on[t]['path']['harq'] == 't%d,rv%d,skip=%d' % (t, RV[t], t > 0)
    # the classes as constructed, from the run's own tx_used
    used, ok = on[-1]['tx_used'], on[-1]['crc_ok']
    hi_tx = TBS[tb]['hi_tx']
    later = set()
    for g, grp in enumerate(groups):
        u, o = used[g * 64:(g + 1) * 64], ok[g * 64:(g + 1) * 64]
        if grp[0] == 'fin':
            assert (u == hi_tx).all() and o.all(), (tag, g)
        elif grp[0] == 'full':
            assert (u == MAX_TX).all() and not o.any(), (tag, g)
        else:
            _, hi, ladder, lo = grp
            assert int(np.sum((o != 0) & (u == hi_tx))) >= hi and int(np.sum(o == 0)) >= lo, (tag, g, u, o)
            later |= set(u[(o != 0) & (u > hi_tx)].tolist())
    print('states', tag, states, 'acknowledged later after', sorted(later), 'transmissions')
    assert len(later) >= 2, (tag, later)           # the ladder spreads acknowledgements over the later rounds
    if name in PACKS:
        packed = [on[t]['info'] for t in range(MAX_TX) if on[t]['info']['state'] == 'packed']
        assert packed and all(i['P'] == PACKS[name] and i['A'] % 64 and i['P'] < i['M'] for i in packed), (tag, packed)
    elif name == 'in_place':
        assert all(i['info']['M'] == 2 and i['info']['P'] == 2 for i in on[1:]), tag
    else:
        assert all(i['info']['M'] == 3 and i['info']['P'] == 2 and cap == 1 for i in on[1:]), tag


@pytest.mark.parametrize('mode', ['LTE_HARQ_SKIP=0', 'decoder mode 0'])
def test_plain_rounds_stay_exact(C, monkeypatch, mode):
    """Without the skip-aware decoders no round packs: bit for bit the setting off, bits_rx included."""
    from lte_phy import channel_coding as cc
    clear_switches(monkeypatch)
    tb, max_frames, _ = CASES['partly']
    bits, snrs = inputs('partly')
    try:
        if mode == 'decoder mode 0':
            cc.set_decoder_mode(False)
        else:
            monkeypatch.setenv('LTE_HARQ_SKIP', '0')
        off, on, _ = both(C, tb, 'f64', max_frames, snrs, seed=tb, bits=bits)
    finally:
        cc.set_decoder_mode(True)
    states = check_on_against_off(C, off, on, 2, mode, skip_aware=False, identical=True)
    assert states == ['none', 'in_place', 'in_place', 'in_place']
    assert on[3]['path']['harq'] == 't3,rv1,skip=0' and on[3]['info']['M'] == 3


def test_large_plan_gathers_across_chunk_widths(C, monkeypatch):
    """max_frames 2048: the decoder rows are chunked 32 groups wide, the packed arrays (cap = 8) are not."""
    clear_switches(monkeypatch)
    rs = np.random.RandomState(5)
    B = 2048 - 37
    kinds = [FIN, mix(44, 8, 12), FULL, mix(40, 10, 14)]
    snrs = []
    for g in range(-(-B // 64)):
        valid = min(64, B - 64 * g)
        k = kinds[g % 4] if valid == 64 else mix(15, 6, 6, 27)
        v = np.full(64, HI_DB if k[0] == 'fin' else LO_DB) if k[0] != 'mix' else \
            np.concatenate([np.full(k[1], HI_DB), np.linspace(0.0, 3.0, k[2]), np.full(k[3], LO_DB)])
        snrs.append(v[rs.permutation(len(v))])
    snrs = np.concatenate(snrs)
    assert len(snrs) == B
    for prec in ('f64', 'f32'):
        off, on, plan = both(C, 435, prec, 2048, snrs, seed=11)
        states = check_on_against_off(C, off, on, 8, ('large', prec))
        assert states[1:] == ['packed'] * 3 and on[1]['info']['M'] == 16 and 1 < on[1]['info']['P'] <= 8, on[1]['info']


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_scaled_decoders(C, monkeypatch, prec):
    clear_switches(monkeypatch)
    tb, max_frames, _ = CASES['partly']
    bits, snrs = inputs('partly')
    off, on, plan = both(C, tb, prec, max_frames, snrs, scale=0.75, seed=tb, bits=bits)
    assert plan.turbo_scale == 0.75 and on[1]['path']['ext'] == '0.75'
    states = check_on_against_off(C, off, on, 2, ('scaled', prec))
    assert 'packed' in states


def test_a_second_process_starts_clean(C, monkeypatch):
    from lte_phy import engine
    clear_switches(monkeypatch)
    tb, max_frames, _ = CASES['two_packed']
    bits, snrs = inputs('two_packed')
    engine.clear_cache()
    plan = make_plan(C, tb, 'f64', max_frames, True)
    first = rounds(plan, snrs, seed=1, bits=bits)
    assert any(r['info']['state'] == 'packed' for r in first)
    bits2, snrs2 = inputs('partly')
    again = rounds(plan, snrs2, seed=2, bits=bits2)
    engine.clear_cache()
    fresh = make_plan(C, tb, 'f64', max_frames, True)
    assert fresh is not plan
    new = rounds(fresh, snrs2, seed=2, bits=bits2)
    for t in range(MAX_TX):
        for k in KEYS + ('bits_rx',):
            assert np.array_equal(again[t][k], new[t][k]), (t, k)
        assert again[t]['info'] == new[t]['info'] and again[t]['harq_info'] == new[t]['harq_info'], t
    assert any(r['info']['state'] == 'packed' for r in new)
    # switched off on the same plan, a process is the plain one again (and its path says so)
    plan.set_harq_repack(False)
    off = rounds(plan, snrs2, seed=2, bits=bits2)
    assert all(r['info'] is None and 'harq_repack' not in r['path'] for r in off)
    for t in range(MAX_TX):
        for k in KEYS:
            assert np.array_equal(off[t][k], new[t][k]), (t, k)
        assert off[t]['harq_info'] == new[t]['harq_info']


def test_setting_changed_between_rounds(C, oracle, monkeypatch):
    """The setting changed between rounds of a process under way, on a plan made
    with it off.  Switched on after round 1 (first use: the packed arrays are
    allocated and the latch's flags move), round 2 has no index yet and runs in
    place on the flags alone, round 3 follows the rule on round 2's verdicts; a
    second process switches off again after round 2.  Every round of both equals
    the process that never had the setting."""
    from lte_phy import engine
    clear_switches(monkeypatch)
    tb, max_frames, _ = CASES['partly']
    bits, snrs = inputs('partly')
    off, _, _, cap = case_runs(C, oracle, 'partly', 'f64')
    B = len(snrs)
    G = -(-B // 64)
    for back_off in (False, True):
        engine.clear_cache()
        plan = make_plan(C, tb, 'f64', max_frames, False)
        got = []
        for t in range(MAX_TX):
            if t == 2:
                plan.set_harq_repack(True)
            if t == 3 and back_off:
                plan.set_harq_repack(False)
            got.append(one_round(plan, t, snrs, seed=tb, bits=bits))
        for t in range(MAX_TX):
            a, b = off[t], got[t]
            tag = (back_off, t)
            for k in KEYS:
                assert np.array_equal(a[k], b[k]), (tag, k)
            assert a['harq_info'] == b['harq_info'], tag
            active = got[t - 1]['crc_ok'] == 0 if t else np.ones(B, dtype=bool)
            assert np.array_equal(a['bits_rx'][active], b['bits_rx'][active]), tag
        for t in (0, 1):
            assert got[t]['info'] is None and 'harq_repack' not in got[t]['path'], (back_off, t)
        # right after switching on: no index exists yet
        info, prev = got[2]['info'], got[1]['crc_ok']
        finished = sum(1 for g in range(G) if prev[g * 64:(g + 1) * 64].all())
        assert got[2]['path']['harq_repack'] == '1' and info['on'] and info['cap'] == cap, (back_off, info)
        assert (info['state'], info['M'], info['A'], info['P']) == ('in_place', 0, 0, 0), (back_off, info)
        assert finished >= 1 and info['waves'] == G - finished, (back_off, info, finished)
        if back_off:
            assert got[3]['info'] is None and 'harq_repack' not in got[3]['path']
            continue
        # the next round: the rule's numbers on round 2's verdicts
        info, prev = got[3]['info'], got[2]['crc_ok']
        want = C.harq_repack_rule(prev, cap)
        assert want == RM.rule(prev, cap)
        assert got[3]['path']['harq_repack'] == '1'
        assert (info['M'], info['A'], info['P']) == (want['M'], want['A'], want['P']), (info, want)
        assert info['state'] == ('packed' if want['pack'] else 'in_place') and info['waves'] == want['waves_on'], \
            (info, want)
        assert want['pack'] and info['P'] == PACKS['partly']     # (the case is built to pack)


def test_a_packed_round_runs_under_the_existing_timers(C, monkeypatch):
    """No new timing slot.  A round that packs brackets the gather, the scatter,
    the latch and the index under `harq` and its two decoder launches under one
    `turbo` bracket; a round in place adds the index alone; setting off: the latch."""
    from lte_phy import engine
    clear_switches(monkeypatch)
    got = {}
    for name, repack in (('partly', True), ('in_place', True), ('partly', False)):
        tb, max_frames, _ = CASES[name]
        bits, snrs = inputs(name)
        engine.clear_cache()
        plan = make_plan(C, tb, 'f64', max_frames, repack)
        plan.harq_round(0)
        plan.run(snrs, seed=tb, bits=bits)
        plan.timing(True)
        plan.timing_reset()
        plan.harq_round(1)
        r = plan.run(snrs, seed=tb, bits=bits)
        plan.timing(False)
        got[name, repack] = (plan.timing_read(), r.get('harq_repack_info'))
    (packed, pi), (inplace, ii), (off, _) = got['partly', True], got['in_place', True], got['partly', False]
    assert pi['state'] == 'packed' and ii['state'] == 'in_place'
    assert list(packed) == list(off) == list(inplace)
    assert (packed['harq'][1], inplace['harq'][1], off['harq'][1]) == (4, 2, 1)
    assert packed['turbo'][1] == inplace['turbo'][1] == off['turbo'][1] == 1
    for k in packed:
        if k not in ('harq', 'turbo'):
            assert packed[k][1] == off[k][1], k


def test_refusals_and_memory(C, monkeypatch):
    """A plan without HARQ refuses the setting; the packed arrays are held only
    by a plan that switched it on, and lte_plan_destroy gives everything back."""
    from lte_phy import engine
    import lte_phy
    clear_switches(monkeypatch)
    lib = C.load()
    engine.clear_cache()
    gc.collect()
    start = lib.lte_device_bytes_held()
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=1.25, modulation='QPSK'), channel_type='awgn')
    plain = sim._plan(C.CHAIN_CODED, 0, 435, max_frames=70, iters=ITERS)
    assert lib.lte_plan_set_harq_repack(plain.h, 1) == C.LTE_EINVAL and b'HARQ' in lib.lte_last_error()
    info = np.zeros(7, dtype=np.int64)
    assert lib.lte_plan_harq_repack_info(plain.h, C.ptr(info, C.c_i64), 7) == C.LTE_EINVAL
    assert lib.lte_plan_harq_repack(plain.h) == 0
    with pytest.raises(ValueError):
        plain.set_harq_repack(True)
    del plain
    engine.clear_cache()
    gc.collect()
    assert lib.lte_device_bytes_held() == start
    off = make_plan(C, 435, 'f64', 320, False)
    held_off = lib.lte_device_bytes_held() - start
    on = make_plan(C, 435, 'f64', 320, True)
    held_on = lib.lte_device_bytes_held() - start - held_off
    assert held_off > 0 and held_on > held_off          # the packed rows, checkpoints, words and index
    off.set_harq_repack(True)                            # first use allocates; off again frees nothing
    assert lib.lte_device_bytes_held() - start == 2 * held_on
    off.set_harq_repack(False)
    assert lib.lte_device_bytes_held() - start == 2 * held_on
    bits, snrs = inputs('two_packed')
    assert any(r['info']['state'] == 'packed' for r in rounds(on, snrs, seed=1, bits=bits))
    del off, on
    engine.clear_cache()
    gc.collect()
    assert lib.lte_device_bytes_held() == start
