"""GPU: the coded SISO pipeline (LTE_CODED_PIPE, run_siso_pipe in lte_capi.hip):
the batch queued in slices of whole 64-frame groups, the front end of slice
i + 1 beside the decode of slice i on two decoder streams.

The contract is equality, not closeness: the sliced run launches the same
kernels on the same per-frame arguments (Philox keys are the frame ids) and the
same 64-frame decoder groups, so counts, frame_errors and crc_ok are exactly
those of the same plan with LTE_CODED_PIPE=0.  Every comparison also checks
lte_plan_pipe_info: a silent fall-back to the serial path would pass the
equality on its own.

  (1) the bench chain, chunk width 32: ragged last group, one-frame last slice,
      exactly two slices, a short second slice; f64 and f32
  (2) chunk width 1 (a plan under 32 groups)      (3) a non-2048 transmitter
  (4) state across runs on one plan               (5) the fall-backs
  (6) the timers                                  (7) frames against the oracle
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TB = 27760
SEED = 0x5EED
SNRS = np.arange(0, 31, 2, dtype=np.float64)
KEYS = ('counts', 'frame_errors', 'crc_ok')


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


def make_plan(C, prec='f64', bw=20.0, mod='64-QAM', tb=TB, max_frames=6244, iters=2, **kw):
    import lte_phy
    sim = lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=bw, modulation=mod), channel_type='rayleigh_mp',
                                itu_profile='Pedestrian_A', precision=prec)
    return sim._plan(C.CHAIN_CODED, 0, tb, max_frames=max_frames, iters=iters, **kw)


def run(plan, monkeypatch, pipe, groups, B, id0=0, **kw):
    """B frames with ids id0 .., SNR index = frame id mod 16 on 0:2:30 dB (the
    bench's rule) -> (the outputs, pipe_info of the run)."""
    monkeypatch.setenv('LTE_CODED_PIPE', '1' if pipe else '0')
    monkeypatch.setenv('LTE_CODED_PIPE_GROUPS', str(groups))
    ids = np.arange(B, dtype=np.uint64) + np.uint64(id0)
    si = (ids % np.uint64(len(SNRS))).astype(np.int32)
    r = plan.run(SNRS[si], snr_index=si, n_snr=len(SNRS), seed=SEED, frame_ids=ids, **kw)
    return r, plan.pipe_info()


_SERIAL = {}


def serial(plan, tag, monkeypatch, groups, B, id0=0):
    """The serial twin of a run, made once per (plan, B, id0) and never changed."""
    key = (tag, B, id0)
    if key not in _SERIAL:
        r, info = run(plan, monkeypatch, False, groups, B, id0)
        assert info == {'slices': 0, 'groups': 0, 'reason': 'off'}, info
        _SERIAL[key] = {k: r[k].copy() for k in KEYS}
    return _SERIAL[key]


def assert_equal(r, ref, what):
    for k in KEYS:
        assert np.array_equal(r[k], ref[k]), (what, k, np.flatnonzero(np.ravel(r[k] != ref[k]))[:8].tolist())


def check_on_off(plan, tag, monkeypatch, groups, B, slices, id0=0):
    ref = serial(plan, tag, monkeypatch, groups, B, id0)
    r, info = run(plan, monkeypatch, True, groups, B, id0)
    assert info['slices'] >= 2 and info['reason'] == 'pipelined', info
    assert (info['slices'], info['groups']) == slices, info
    assert_equal(r, ref, (tag, B, id0))
    return r


# ---------------------------------------------------------------------------
# (1) the bench chain: 20 MHz 64-QAM PedA, TB 27 760, a plan of 98 groups (chunk
# width 32), slices of 32 groups = 2 048 frames
@pytest.mark.parametrize('prec,B,slices', [
    ('f64', 6244, (4, 32)),    # 98 groups: three slices and one of two groups, the last group ragged (36 frames)
    ('f64', 4160, (3, 32)),    # 65 groups: the last slice one full group
    ('f64', 4097, (3, 32)),    # the last slice one frame
    ('f64', 4096, (2, 32)),    # exactly two slices
    ('f64', 2112, (2, 32)),    # a short second slice (one group)
    ('f32', 4160, (3, 32))])
def test_bench_chain_chunk32(C, monkeypatch, prec, B, slices):
    plan = make_plan(C, prec)
    r = check_on_off(plan, ('c32', prec), monkeypatch, 32, B, slices)
    assert r['counts'][:, 1].sum() == B * TB and r['counts'][:, 3].sum() == B


_FULL8 = {}


def full8(C, monkeypatch):
    """B = 6 244 at 8 iterations, pipelined (checked against its serial twin): shared with the oracle check."""
    if not _FULL8:
        plan = make_plan(C, 'f64', iters=8)
        r = check_on_off(plan, ('c32', 'f64', 8), monkeypatch, 32, 6244, (4, 32), id0=7 * 65536)
        _FULL8.update({k: r[k].copy() for k in KEYS})
    return _FULL8


def test_bench_chain_eight_iterations(C, monkeypatch):
    r = full8(C, monkeypatch)
    assert set(np.unique(r['crc_ok']).tolist()) == {0, 1}      # failing and passing blocks both present
    assert r['frame_errors'][r['crc_ok'] == 1].sum() == 0


# ---------------------------------------------------------------------------
# (2) chunk width 1: the same chain in a plan of 10 groups, slices of 3 groups
@pytest.mark.parametrize('B,slices', [(640, (4, 3)), (600, (4, 3)), (193, (2, 3))])
def test_chunk_width_one(C, monkeypatch, B, slices):
    plan = make_plan(C, 'f64', max_frames=640)
    check_on_off(plan, 'c1', monkeypatch, 3, B, slices, id0=31)


# (3) 5 MHz 16-QAM: N = 512, four frames per transmitter block, the run-time-N k_ofdm_txf instance
def test_other_transmitter(C, monkeypatch):
    plan = make_plan(C, 'f64', bw=5.0, mod='16-QAM', tb=6000, max_frames=640)
    r = check_on_off(plan, 'n512', monkeypatch, 3, 450, (3, 3), id0=900)      # 8 groups: 3 + 3 + 2, the last ragged
    assert r.path['tx'] == 'k_ofdm_txf' and r.path['rx'] == 'k_rx_frame' and r.path['dematch'] == 'zn'


# (4) one plan: on, off, on, on with different sizes and frame ids
def test_state_across_runs(C, monkeypatch):
    plan = make_plan(C, 'f64', max_frames=640)
    seq = [(True, 640, 100), (False, 600, 2000), (True, 193, 40000), (True, 500, 77)]
    got = []
    for pipe, B, id0 in seq:
        r, info = run(plan, monkeypatch, pipe, 3, B, id0)
        assert (info['slices'] >= 2) == pipe and (info['slices'] == 0) == (not pipe), (pipe, info)
        got.append({k: r[k].copy() for k in KEYS})
    for (pipe, B, id0), r in zip(seq, got):
        assert_equal(r, serial(plan, 'c1', monkeypatch, 3, B, id0), (pipe, B, id0))


# (5) what keeps a run serial under LTE_CODED_PIPE=1
@pytest.mark.parametrize('case', ['cap_llr', 'bits', 'early_stop', 'harq', 'one_slice'])
def test_fallbacks(C, monkeypatch, case):
    kw, B, groups = {}, 450, 3
    reason = {'cap_llr': 'capture', 'bits': 'inject', 'early_stop': 'decoder', 'harq': 'decoder',
              'one_slice': 'one_slice'}[case]
    if case == 'early_stop':
        plan = make_plan(C, 'f64', max_frames=640, early_stop=True)
    elif case == 'harq':
        plan = make_plan(C, 'f64', max_frames=640, harq=dict(max_tx=2))
    else:
        plan = make_plan(C, 'f64', max_frames=640)
    if case == 'cap_llr':
        kw['capture'] = ('llr',)
    if case == 'bits':
        kw['bits'] = np.random.RandomState(5).randint(0, 2, (B, TB)).astype(np.uint8)
    if case == 'one_slice':
        B, groups = 192, 3
    ref, info0 = run(plan, monkeypatch, False, groups, B, 11, **kw)
    assert info0 == {'slices': 0, 'groups': 0, 'reason': 'off'}
    r, info = run(plan, monkeypatch, True, groups, B, 11, **kw)
    assert info == {'slices': 0, 'groups': 0, 'reason': reason}, info
    assert_equal(r, ref, case)
    if case == 'cap_llr':
        assert np.array_equal(r['llr'], ref['llr'])


# (6) timers: `turbo` is one interval and one launch per pipelined run; the front-end stages keep their names
def test_timers(C, monkeypatch):
    plan = make_plan(C, 'f64', max_frames=640)
    plan.timing_reset()
    plan.timing(True)
    try:
        run(plan, monkeypatch, False, 3, 640, 5)
        ser = plan.timing_read()
        plan.timing_reset()
        k = 3
        for i in range(k):
            _, info = run(plan, monkeypatch, True, 3, 640, 5 + i)
            assert info['slices'] == 4
        pip = plan.timing_read()
    finally:
        plan.timing(False)
        plan.timing_reset()
    assert ser['turbo'][1] == 1 and pip['turbo'][1] == k and pip['turbo'][0] > 0, (ser, pip)
    front = [n for n, (ms, nl) in ser.items() if nl > 0]
    assert {'payload', 'encode', 'ofdm_tx', 'fading', 'channel', 'rx_data', 'dematch', 'crc_count',
            'accumulate'} <= set(front)
    for n in front:
        assert pip[n][1] >= k * ser[n][1] and pip[n][0] > 0, (n, ser[n], pip[n])
    for n in ('ofdm_tx', 'fading', 'channel', 'rx_data', 'dematch'):       # one bracket per slice
        assert pip[n][1] == 4 * k * ser[n][1], (n, ser[n], pip[n])


# (7) eight frames over all four slices of the 8-iteration run against the float64 oracle on its Philox restatement
def test_oracle_spot_check(C, monkeypatch):
    from oracle import philox as P
    r = full8(C, monkeypatch)
    sel = np.array([5, 2047, 2048, 3001, 4095, 4096, 6144, 6243])
    assert sorted(set((sel // 2048).tolist())) == [0, 1, 2, 3]
    orc = np.array([P.BENCH_FRAMES[2](int(f)) for f in sel + 7 * 65536])
    assert np.array_equal(r['frame_errors'][sel], orc[:, 0]), (r['frame_errors'][sel].tolist(), orc[:, 0].tolist())
    assert np.array_equal(r['crc_ok'][sel], orc[:, 1]), (r['crc_ok'][sel].tolist(), orc[:, 1].tolist())
