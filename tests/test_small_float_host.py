"""The host side of the small-scene path's fp32 shape (csrc/render_small.hip: the 1024-thread workgroup holds the nodes as fp32, the
256-thread workgroup holds none), without a GPU: the budget's arithmetic against the formulas stated here, the padding that keeps a
second 256-thread workgroup off a CU, and the few trees the two-copy budget admits and this one does not; the new hooks are declared."""
import numpy as np

from acgpathtracing_amd import _build, _native

CU_LDS = 160 * 1024
MAX_NODES = 2048


def kb(b):
    return (b + 1023) // 1024 * 1024


def old_budget(n, s):
    """the two-copy budget of tests/test_small_kernel_host.py: (big, little, eligible)"""
    big = 16 * s * 128 + n * 32 + 256 + 16 * 320
    little = 4 * s * 128 + n * 32 + 256 + 4 * 320
    return big, little, kb(big) + kb(little) <= CU_LDS and big + 2 * little > CU_LDS


def float_budget(n, s, cu=CU_LDS):
    """(big, little, the 256-thread launch's request, fits): fp32 nodes are 64 bytes each and only the 1024-thread workgroup holds them"""
    big = 16 * (s * 128 + 320) + n * 64 + 256
    little = 4 * (s * 128 + 320) + 256
    request = max(little, ((cu - big) // 2 + 16) // 16 * 16) if big < cu else little
    return big, little, request, kb(big) + kb(little) <= cu


def ask(n, s, cu=CU_LDS):
    out = np.zeros(4, np.uint64)
    assert _native.hip().pt_debug_small_float_budget(n, s, cu, out.ctypes.data) == 0
    return int(out[0]), int(out[1]), int(out[2]), bool(out[3])


def ask_old(n, s):
    out = np.zeros(5, np.uint64)
    assert _native.hip().pt_debug_small_budget(n, n + 1, s, CU_LDS, out.ctypes.data) == 0
    return bool(out[2])


def test_cornell_values():
    big, little, request, fits = ask(1263, 24)
    assert (big, little) == (135360, 13824) and fits
    assert big + little == 149184 == sum(old_budget(1263, 24)[:2])          # the CU's total is the two-copy shape's
    assert request == 14256 and request % 16 == 0                           # (163 840 - 135 360) / 2 = 14 240, and one 16-byte step
    assert big + request <= CU_LDS < big + 2 * request
    assert CU_LDS - big >= 2 * little                                       # unpadded, two small workgroups would fit beside the large one


def test_arithmetic_and_padding_over_the_range():
    """every (N, S) the references and the stack sizes allow: the hook is the formula; where the shape fits, one padded 256-thread
    workgroup fits beside the 1024-thread one counted in whole KB, and two never do, whatever the allocation granule"""
    for s in range(4, 29, 4):
        for n in list(range(1, MAX_NODES + 1, 7)) + [MAX_NODES]:
            got = ask(n, s)
            assert got == float_budget(n, s), (n, s)
            big, little, request, fits = got
            assert request >= little and request % 16 == 0
            if fits:
                assert big + 2 * request > CU_LDS, (n, s)                   # the padding rule
                assert kb(big) + kb(request) <= CU_LDS, (n, s)              # ... and the padded request still fits
                assert request == little or 2 * request - (CU_LDS - big) <= 32      # "just over" half of what is left
    assert not ask(1263, 24, 64 * 1024)[3]                                   # a CU with 64 KB of LDS
    assert ask(1, 4, 4096)[2] == ask(1, 4, 4096)[1]                          # no room at all: nothing to pad to


def test_trees_the_two_copy_budget_admits_and_this_one_does_not():
    """S = 4 ... 28, N = 1 ... 2048: the pairs small_eligible accepts, and those among them whose fp32 shape misses the CU — by KB
    rounding alone: their bytes are within 2 KB of the limit.  The hooks and the formulas name the same set."""
    eligible, rejected, rejected_by_hook = 0, [], []
    for s in range(4, 29, 4):
        for n in range(1, MAX_NODES + 1):
            if not old_budget(n, s)[2]:
                continue
            eligible += 1
            if not float_budget(n, s)[3]:
                rejected.append((n, s))
            assert ask_old(n, s)
            if not ask(n, s)[3]:
                rejected_by_hook.append((n, s))
    assert rejected_by_hook == rejected
    assert eligible == 4594 and len(rejected) == 20
    assert (1965, 12) in rejected and (1805, 16) in rejected and (1327, 28) in rejected
    for n, s in rejected:
        big, little, _, _ = float_budget(n, s)
        assert big + little <= CU_LDS < kb(big) + kb(little)                 # rounding only


def test_hooks_are_declared_and_the_kernel_hash_stays():
    assert _build.kernel_source_hash() == "0ae80f7fe3d9b38b" and len(_build.KERNEL_SOURCES) == 10
    for s in ("pt_debug_small_shape", "pt_debug_small_float_budget", "pt_debug_small_staged"):
        assert s in _native.TEST_SYMBOLS and hasattr(_native.hip(), s)
