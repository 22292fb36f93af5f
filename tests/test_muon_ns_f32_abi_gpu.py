"""The fp32 Newton-Schulz entry points (csrc/muon_ns_f32.hip and the fp32 forms of the apply / dual-dot
launches) validate their arguments themselves, as their siblings do (tests/test_c_abi_errors.py):
PCV_EINVAL for a null table, nmats <= 0, a negative ns_steps and ns_b == 0, before any launch.  Raw
ctypes with fake device addresses, which a launch would fault on."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

A16 = 0x10000
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (shares torch's HIP runtime, as in production)
    from plaincv_amd import hip
    return hip.load()


def P(x):
    return ctypes.c_void_p(x) if x else None


def _ns(lib, recs=A16, nmats=1, tiles=A16, nsym=1, nupd=1, ns_b=-4.775, ns_steps=5):
    return lib.pcv_muon_ns_f32(P(recs), nmats, P(tiles), nsym, nupd, 1e-8, 3.4445, ns_b, 2.0315, ns_steps, None)


def test_ns_f32_chain(lib):
    assert lib.pcv_muon_ns_f32_rec_size() == 64
    assert lib.pcv_muon_ns_f32_tile() == 32
    assert _ns(lib, recs=0) == EINVAL
    assert _ns(lib, tiles=0) == EINVAL
    assert _ns(lib, nmats=0) == EINVAL and _ns(lib, nmats=-3) == EINVAL
    assert _ns(lib, nsym=0) == EINVAL and _ns(lib, nupd=0) == EINVAL
    assert _ns(lib, ns_steps=-1) == EINVAL
    assert _ns(lib, ns_b=0.0) == EINVAL
    assert _ns(lib, ns_steps=0, nmats=0) == EINVAL


def test_apply_and_dual_dot_f32(lib):
    for mats, nmats, elems in [(0, 1, 1024), (A16, 0, 1024), (A16, -1, 1024), (A16, 1, 1 << 31)]:
        assert lib.pcv_muon_apply_f32(P(mats), nmats, elems, 1e-2, 0.1, 1, 1, None) == EINVAL
        assert lib.pcv_muon_apply_dual_f32(P(mats), nmats, elems, 1e-2, 0.1, 1, 1, P(A16), None) == EINVAL
        assert lib.pcv_muon_dual_dot_f32(P(mats), nmats, elems, 0.95, 1, P(A16), None, P(A16), None) == EINVAL
    assert lib.pcv_muon_dual_dot_f32(P(A16), 1, 1024, 0.95, 1, None, None, P(A16), None) == EINVAL   # no step
    assert lib.pcv_muon_dual_dot_f32(P(A16), 1, 1024, 0.95, 1, P(A16), None, None, None) == EINVAL   # no dual
