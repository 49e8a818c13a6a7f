"""The box test of the small-scene render kernel (csrc/small_slab.h: near and far by one fma each) in its own right, end to end through
pack_centre_half and setup_ray_hc: pt_selftest op 42 on the packed fp16 words (slab_hcf), op 43 on the operands converted to fp32 as
the kernel stages them (slab_hcf_f32).  On the case generator of test_gpu_golden.test_gpu_fp16_slab_is_conservative (a copy of it in
tests/small_slab_cases.py), 2^20 cases a set: no ray that meets the unpadded box is rejected; rays that miss the inflated box are
(almost) never accepted; the two operand forms give the same bits."""
import numpy as np
import pytest

import acgpathtracing_amd as pt
import small_slab_cases as cases
from acgpathtracing_amd import _native

pytestmark = pytest.mark.gpu

N = 1 << 20


@pytest.fixture(scope="module")
def ctx(built):
    state = pt.PathTracerState()
    pt.createDeviceContext(state, 0)
    yield state.context
    _native.hip().pt_destroy(state.context)


@pytest.fixture(scope="module")
def sets():
    return cases.case_sets(N)


def run(ctx, op, rec):
    L = _native.hip()
    out = np.zeros((len(rec), 3), np.uint32)
    assert L.pt_selftest(ctx, op, rec.ctypes.data, len(rec), out.ctypes.data) == 0, L.pt_last_error(ctx)
    return out


@pytest.mark.parametrize("name", ["one_scale", "squeezed", "flat"])
def test_fused_slab_is_conservative(ctx, sets, name):
    rec, must, wide, least = sets[name]
    assert len(rec) == N and must.mean() > least, "the case generator lost its hits: %.3f" % must.mean()
    assert (~wide).mean() > 0.05
    packed, staged, old = run(ctx, 42, rec), run(ctx, 43, rec), run(ctx, 41, rec)
    accepted = packed[:, 0] == 1
    missed = must & ~accepted
    differ = (packed[:, 0] != old[:, 0])
    print("%s: %d of %d rays must hit, %d rejected; %.4f %% of the rays that miss the box inflated by 2 %% of the scene are accepted (slab_hc: %.4f %%), "
          "%.1f %% of all rays; %d decisions differ from slab_hc's" % (name, must.sum(), N, missed.sum(), 100 * accepted[~wide].mean(),
                                                                       100 * (old[~wide, 0] == 1).mean(), 100 * accepted.mean(), differ.sum()))
    assert set(np.unique(packed[:, 0])) <= {0, 1}
    assert not missed.any(), "%s: box test rejected %d of %d rays that meet the unpadded box, first: %s" % (name, missed.sum(), must.sum(), rec[np.argmax(missed)])
    assert accepted[~wide].mean() < 1e-3, accepted[~wide].mean()
    # fp16 -> fp32 is exact: accepted, near and far of the two operand forms are the same words
    assert np.array_equal(packed, staged), "%d records differ between the packed and the staged form, first: %s" % (
        (packed != staged).any(axis=1).sum(), rec[np.argmax((packed != staged).any(axis=1))])
