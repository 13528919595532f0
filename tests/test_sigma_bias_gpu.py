"""GPU: d sigma_layer.bias of the fused trainer's backward is ONE number, the sum of d_sigma, and is taken in float64 in a
fixed order (`sigma_bias_kernel`, csrc/mlp_train.hip): on a mask whose summands cancel 4 148-fold (m % 7 == 0 of 385
samples, the case tests/test_sparse_backward_gpu.py describes at OWN) it is right to a float32 half-ulp of ITSELF in both
modes and the same bits at every repetition, whatever ran before -- a float32 column sum by atomics gives 2.4e-6 or 7e-5
by the order of its additions."""
import pytest
import torch

from test_sparse_backward_gpu import Trainer, references

pytestmark = pytest.mark.gpu
KEY = "net.sigma_layer.bias"


@pytest.mark.parametrize("mode", ["dense", "sparse"])
def test_the_cancelling_sum_is_exact_and_repeats(mode):
    t = Trainer(mode == "sparse")
    _, _, _, w_sig, g64, _ = references("every7")
    exact = w_sig.double().sum()
    assert abs(float(g64[KEY]) - float(exact)) <= 1e-12 * float(w_sig.abs().sum())        # the layer's bias gradient IS that sum
    assert float(w_sig.abs().sum()) > 4000 * abs(float(exact))                               # ... and it cancels
    seen = []
    for fill in (None, 0xFF, 0x00, None, None):                   # other workspaces, other allocations in between
        seen.append(t.run("every7", fill=fill)[KEY])
        torch.empty(1 << 20, device="cuda").fill_(1.0)
    t.t.status()
    for g in seen:
        assert g.shape == (1,) and torch.equal(g.view(torch.int32), seen[0].view(torch.int32))
    # the float64 sum rounded once: within a float32 half-ulp of the host's float64 sum (taken in another order)
    assert abs(seen[0].item() - float(exact)) <= 2.0 ** -24 * abs(float(exact)) * (1 + 1e-6)
    assert abs(seen[0].item() - float(g64[KEY])) <= 2e-5 * abs(float(g64[KEY]))
