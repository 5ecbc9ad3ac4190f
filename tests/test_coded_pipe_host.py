"""CPU: the coded SISO pipeline's interface -- the slicing rule
(lte_coded_pipe_slices: groups, chunk width, LTE_CODED_PIPE_GROUPS -> (first
group, groups) per slice), the C ABI additions and the refusals that return
before a device is touched.  The pipeline itself is checked on the GPU in
tests/test_gpu_coded_pipe.py."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ['lte_plan_pipe_info', 'lte_coded_pipe_slices']


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    return _capi


def test_header_declares_and_library_exports(C):
    text = open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()
    lib = C.load()
    for name in NEW_SYMBOLS:
        assert re.search(r'^int %s\(' % name, text, re.M), name
        assert getattr(lib, name).argtypes == C._SIGS[name][1], name
    assert re.search(r'^#define LTE_ABI_VERSION 3$', text, re.M)       # additions only
    assert lib.lte_version() == 3


def check_slices(sl, groups, chunk, knob):
    per = -(-knob // chunk) * chunk                                    # the knob rounded up to the chunk width
    assert len(sl) == -(-groups // per)
    nxt = 0
    for i, (g0, G) in enumerate(sl):
        assert g0 == nxt and g0 % chunk == 0, (i, g0)                  # no gap, no overlap, chunk aligned
        assert G == (per if i < len(sl) - 1 else groups - g0) and 1 <= G <= per   # whole slices, then the rest
        nxt = g0 + G
    assert nxt == groups                                               # full cover


@pytest.mark.parametrize('groups,chunk,knob', [
    (1024, 32, 256), (1024, 32, 224), (1024, 32, 352), (1024, 32, 512), (1024, 32, 1024), (1024, 32, 4096),
    (98, 32, 32), (65, 32, 32), (64, 32, 32), (33, 32, 32), (32, 32, 32), (98, 32, 1), (98, 32, 33), (1000, 32, 250),
    (10, 1, 3), (10, 1, 1), (4, 1, 3), (3, 1, 3), (1, 1, 3), (31, 1, 7), (1, 32, 1)])
def test_slicing_rule(C, groups, chunk, knob):
    check_slices(C.coded_pipe_slices(groups, chunk, knob), groups, chunk, knob)


def test_slicing_rule_examples(C):
    """The cases spelled out: a ragged last slice, a knob that is no multiple of
    the chunk width, exactly two slices, one slice."""
    assert C.coded_pipe_slices(98, 32, 32) == [(0, 32), (32, 32), (64, 32), (96, 2)]
    assert C.coded_pipe_slices(98, 32, 33) == [(0, 64), (64, 34)]
    assert C.coded_pipe_slices(1024, 32, 352) == [(0, 352), (352, 352), (704, 320)]
    assert C.coded_pipe_slices(64, 32, 32) == [(0, 32), (32, 32)]
    assert C.coded_pipe_slices(10, 1, 3) == [(0, 3), (3, 3), (6, 3), (9, 1)]
    assert C.coded_pipe_slices(1024, 32, 1024) == [(0, 1024)]


def test_slicing_output_is_cut_to_n_max(C):
    lib = C.load()
    out = np.full((2, 2), -1, dtype=np.int32)
    assert lib.lte_coded_pipe_slices(98, 32, 32, C.ptr(out, C.I32), 2) == 4
    assert out.tolist() == [[0, 32], [32, 32]]
    assert lib.lte_coded_pipe_slices(98, 32, 32, None, 0) == 4


def test_refusals_without_a_device(C):
    lib = C.load()
    out = np.zeros((4, 2), dtype=np.int32)
    for groups, chunk, knob in ((0, 32, 32), (-1, 1, 1), (10, 0, 3), (10, -32, 3), (10, 1, 0), (10, 1, -5)):
        assert lib.lte_coded_pipe_slices(groups, chunk, knob, C.ptr(out, C.I32), 4) == C.LTE_EINVAL
    assert lib.lte_coded_pipe_slices(10, 1, 3, None, 4) == C.LTE_EINVAL
    assert lib.lte_coded_pipe_slices(10, 1, 3, C.ptr(out, C.I32), -1) == C.LTE_EINVAL
    info = np.zeros(3, dtype=np.int64)
    assert lib.lte_plan_pipe_info(None, C.ptr(info, C.c_i64), 3) == C.LTE_EINVAL


def test_reason_names_cover_the_codes():
    """engine.PIPE_REASONS names lte_plan_pipe_info's codes 0 .. 8 in the header's order."""
    from lte_phy import engine
    text = open(os.path.join(ROOT, 'include', 'lte_phy.h')).read()
    doc = text[text.index('The coded SISO pipeline'):text.index('int lte_plan_pipe_info(')]
    assert [int(c) for c in re.findall(r'\b([0-8]) (?:pipelined|LTE_CODED_PIPE is|another|not every|a capture|an inj|HARQ|the batch)', doc)] \
        == list(range(9))
    assert len(engine.PIPE_REASONS) == 9 and engine.PIPE_REASONS[0] == 'pipelined' and engine.PIPE_REASONS[8] == 'one_slice'
