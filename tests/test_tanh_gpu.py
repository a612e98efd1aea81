"""HF.tanh (unet.hip), forward and backward (dx = dy (1 - y^2) from the saved output), on (2, 3, 8, 8)
and (1, 3, 5, 7) with inputs spanning +-12.

The error against fp64 is measured as max |err|; the bar is 4x the error of torch's CPU fp32 tanh on the
same inputs (its forward, and its autograd backward for dx), floored at one fp32 ulp of 1.0 (2^-23).

Measured on an MI355X, max |err| against fp64 (torch CPU fp32 on the same inputs in brackets):
  (2, 3, 8, 8): forward 4.195e-08 (2.990e-08), backward 1.518e-07 (1.518e-07);
  (1, 3, 5, 7): forward 2.914e-08 (2.914e-08), backward 1.468e-07 (1.468e-07).
The test prints the figures on every run.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ULP1 = 2.0 ** -23


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import dsgan_hip
    dsgan_hip.require_gpu()
    yield


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (1, 3, 5, 7)])
def test_tanh_against_fp64(shape):
    from dsgan_hip import functional as HF
    g = torch.Generator().manual_seed(sum(shape))
    n = int(torch.tensor(shape).prod())
    x = (torch.linspace(-12.0, 12.0, n)[torch.randperm(n, generator=g)]).reshape(shape)
    x.view(-1)[0] = 0.0
    gy = torch.randn(shape, generator=g)
    x64 = x.double().requires_grad_()
    y64 = torch.tanh(x64)
    y64.backward(gy.double())
    x32 = x.clone().requires_grad_()
    y32 = torch.tanh(x32)
    y32.backward(gy)
    ref_f = float((y32.detach().double() - y64.detach()).abs().max())
    ref_b = float((x32.grad.double() - x64.grad).abs().max())
    xd = x.to(DEV).requires_grad_()
    y = HF.tanh(xd)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    err_f = float((y.detach().double().cpu() - y64.detach()).abs().max())
    err_b = float((xd.grad.double().cpu() - x64.grad).abs().max())
    print("\n[tanh %s] forward max|err| %.3e (torch CPU fp32 %.3e), backward %.3e (torch CPU fp32 %.3e)"
          % (shape, err_f, ref_f, err_b, ref_b))
    assert float(y.detach().cpu().view(-1)[0]) == 0.0 and float(y.detach().abs().max()) <= 1.0
    assert err_f <= max(4 * ref_f, ULP1), (err_f, ref_f)
    assert err_b <= max(4 * ref_b, ULP1), (err_b, ref_b)
