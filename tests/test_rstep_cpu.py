"""CPU-only: the host surface of the real twin's fused step (csrc/mask.hip: dcs_complex_abs_f32, dcs_rmask_apply_polar_frames_fwd /
_bwd) — argument checks that return before any launch, the ops' refusal of CPU tensors, and R_NETWORK.forward's sigmoid= switch.
No compute call is made here — there is no GPU.  (tests/test_host_cpu.py::test_ctypes_signatures_cover_the_header holds header
and ctypes signatures together.)"""
import ctypes
import inspect
import os

import pytest
import torch

P = ctypes.c_void_p(64)                  # a non-null pointer that is never followed: every call below is rejected first


def test_the_three_entry_points_reject_null_and_bad_arguments_before_any_launch():
    from dcsnet import _lib
    lib = _lib.load()
    assert lib.dcs_abi_version() == 20                                   # new entry points only: no signature changed
    assert lib.dcs_complex_abs_f32(None, P, 10, None) == -1
    assert lib.dcs_complex_abs_f32(P, None, 10, None) == -1
    for n in (0, -3):
        assert lib.dcs_complex_abs_f32(P, P, n, None) == -1
    good = (2, 256, 257, 8)                                              # B, F, Fp, T
    for pair in (0, 1):
        for args in ((None, P, P, P), (P, None, P, P), (P, P, P, None)):                       # M_out alone may be NULL
            assert lib.dcs_rmask_apply_polar_frames_fwd(*args, *good, 1e-6, pair, None) == -1
        for args in ((None, P, P, P, P), (P, None, P, P, P), (P, P, None, P, P), (P, P, P, P, None)):   # g_M alone may be NULL
            assert lib.dcs_rmask_apply_polar_frames_bwd(*args, *good, 1e-6, 1, pair, None) == -1
        for dims in ((0, 256, 257, 8), (-1, 256, 257, 8), (65536, 256, 257, 8), (2, 0, 257, 8), (2, 256, 255, 8), (2, 256, 257, 0),
                     (2, 256, 257, -4)):
            assert lib.dcs_rmask_apply_polar_frames_fwd(P, P, None, P, *dims, 1e-6, pair, None) == -1, dims
            assert lib.dcs_rmask_apply_polar_frames_bwd(P, P, P, None, P, *dims, 1e-6, 1, pair, None) == -1, dims


def test_the_ops_refuse_cpu_tensors():
    from dcsnet import ops, functional as F, DcsHipError
    Y = torch.zeros(2, 256, 8, dtype=torch.complex64)
    D = torch.zeros(2, 256, 8)
    with pytest.raises(DcsHipError, match='no CPU fallback'):
        ops.complex_abs(Y)
    with pytest.raises(DcsHipError, match='no CPU fallback'):
        ops.complex_abs(torch.view_as_real(Y))
    with pytest.raises(DcsHipError, match='no CPU fallback'):
        ops.rmask_apply_polar_frames(torch.view_as_real(Y), D, 257)
    with pytest.raises(DcsHipError, match='no CPU fallback'):
        ops.rmask_apply_polar_frames(torch.view_as_real(Y), D, 257, grad=torch.zeros(4, 8, 257, 2), hermitian=True)
    with pytest.raises(DcsHipError, match='no CPU fallback'):
        F.rmask_apply_polar_wave(Y, D, torch.hann_window(512), torch.ones(32 * 7), 512, 32, 1.0, 1e-6)


def test_rnetwork_forward_takes_the_sigmoid_switch():
    from dcsnet.r_network import R_NETWORK
    from dcsnet.c_network import C_NETWORK
    sig = inspect.signature(R_NETWORK.forward)
    assert list(sig.parameters) == ['self', 'x', 'sigmoid'] and sig.parameters['sigmoid'].default is True
    assert R_NETWORK.supports_raw_forward is True and not getattr(C_NETWORK, 'supports_raw_forward', False)


def test_the_step_switch_and_the_enhancer_classes():
    from dcsnet import network_functions as nf
    from dcsnet.enhance import Enhancer, MagnitudeEnhancer
    assert nf.RSTEP_FUSED == (os.environ.get('DCS_RSTEP_FUSED', '1') != '0')    # the fused route unless switched off
    assert issubclass(MagnitudeEnhancer, Enhancer) and MagnitudeEnhancer.MODES == ('drs', 'dr') and Enhancer.MODES == ('dcs', 'dc')
