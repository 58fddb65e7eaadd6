"""CPU: the reference's ops/functions/ms_deform_attn_func.py on this library.  That module does
`import MultiScaleDeformableAttention as MSDA` (func.py:11) -- resolved by trackformer_amd.dropin -- and its MSDeformAttnFunction
(func.py:14-31) is two calls into it: MSDA.ms_deform_attn_forward(value, shapes, loc, attn, im2col_step) in forward and
MSDA.ms_deform_attn_backward(value, shapes, loc, attn, grad_output, im2col_step) in backward, whose three gradients it returns.
Those calls are made here as it makes them and compared, the way the reference's ops/test.py:23-60 does (forward equality, then
gradients of all three inputs), with the reference's own pure-PyTorch ms_deform_attn_core_pytorch (func.py:34-54): its output and
gradients at these inputs are stored in tests/golden/cross_msda_function_*.npz (tests/golden/make_golden_cross.py).
VERDICT r02 item 6(d)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture()
def msda_module():
    """What `import MultiScaleDeformableAttention as MSDA` gives once the drop-in is installed."""
    import trackformer_amd.dropin as dropin
    saved = sys.modules.pop("MultiScaleDeformableAttention", None)
    dropin.install()
    try:
        yield importlib.import_module("MultiScaleDeformableAttention")
    finally:
        sys.modules.pop("MultiScaleDeformableAttention", None)
        if saved is not None:
            sys.modules["MultiScaleDeformableAttention"] = saved


def test_reference_module_binds_to_this_library(msda_module):
    import trackformer_amd.msda as msda
    assert msda_module.ms_deform_attn_forward is msda.ms_deform_attn_forward
    assert msda_module.ms_deform_attn_backward is msda.ms_deform_attn_backward


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-5)], ids=["f64", "f32"])
def test_reference_autograd_function_runs_on_this_library(msda_module, dtype, tol):
    z = np.load(os.path.join(GOLDEN, "cross_msda_function_%s.npz" % ("f64" if dtype == torch.float64 else "f32")))
    value, loc, attn, w = (torch.from_numpy(z[k]) for k in ("value", "loc", "attn", "w"))
    shapes = torch.from_numpy(z["shapes"])
    assert value.dtype == dtype and shapes.dtype == torch.long
    out = msda_module.ms_deform_attn_forward(value, shapes, loc, attn, 2)                 # func.py:18-19
    out_t = torch.from_numpy(z["out"])                                                    # func.py:34-54
    assert out.shape == out_t.shape and float((out - out_t).abs().max()) < tol
    # d (out * w).sum() / d out = w: the grad_output autograd hands to func.py:27-29
    grads = msda_module.ms_deform_attn_backward(value, shapes, loc, attn, w, 2)
    for a, key in zip(grads, ("grad_value", "grad_loc", "grad_attn")):
        b = torch.from_numpy(z[key])
        assert a.shape == b.shape and a.dtype == dtype
        assert float((a - b).abs().max()) < tol * 10 * max(1.0, float(b.abs().max())), key
