"""CPU: linear.pad_to, the one spelling of the GEMM's granule padding (the rest of the module needs the GPU: tests/test_gpu_linear.py)"""
import torch

from metatransformer_amd.linear import pad_to


def test_aligned_input_comes_back_itself():
    t = torch.randn(16, 24)
    assert pad_to(t, 0) is t and pad_to(t, 1) is t and pad_to(t, -1) is t
    assert pad_to(t, 0, multiple=4) is t and pad_to(t[:, :12], 1, multiple=4).shape == (16, 12)


def test_pads_one_dimension_with_zeros():
    t = torch.randn(5, 27) + 3.0      # (no zeros of its own)
    for dim, shape in ((0, (8, 27)), (1, (5, 32)), (-1, (5, 32)), (-2, (8, 27))):
        p = pad_to(t, dim)
        assert p.shape == shape and p.dtype == t.dtype and p.is_contiguous()
        assert torch.equal(p[:5, :27], t)
        assert not p[5:].any() and not p[:, 27:].any()
    assert pad_to(t, 1, multiple=4).shape == (5, 28)


def test_dim_of_a_3d_tensor_and_dtype():
    t = torch.ones(2, 3, 5, dtype=torch.bfloat16)
    p = pad_to(t, 1)
    assert p.shape == (2, 8, 5) and p.dtype == torch.bfloat16
    assert torch.equal(p[:, :3], t) and not p[:, 3:].any()
    v = torch.ones(7)
    assert torch.equal(pad_to(v, 0), torch.tensor([1.0] * 7 + [0.0]))
