"""GPU: `NetPass.pointwise` and `NetPass.conv3x3` (controlanimate_amd/annotator_base.py) are the direct `kernels.gemm` / `kernels.conv3x3`
calls, bit for bit.  The helpers add views and a taken output, never arithmetic, so the comparison is exact.

Shape: 2 images of 8 x 8 pixels, 64 -> 32 channels.  Cases: a residual, a second source `a2` behind x along K, and `out2d` a 32-column
slice of a 128-column buffer -- the case where a wrong view goes wrong: the columns on either side of the slice must keep their fill.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, H, W, CIN, COUT = 2, 8, 8, 64, 32
M = N * H * W


def _rnd(seed, *shape, dtype=torch.float16):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


@pytest.fixture(scope="module")
def net():
    from controlanimate_amd.annotator_base import PackedNetwork

    class Net(PackedNetwork):
        device, dtype = DEV, torch.float16

        def __init__(self):
            self._ws = {}

    n = Net()
    n.ws = n._workspace("ws", lambda dev: {})
    return n


def test_pointwise_equals_the_gemm(net):
    from controlanimate_amd import kernels as K
    x, wt, bias, res = _rnd(1, N, H, W, CIN), _rnd(2, COUT, CIN) / 8, _rnd(3, COUT, dtype=torch.float32), _rnd(4, N, H, W, COUT)
    a2, wt2 = _rnd(5, N, H, W, 16), _rnd(6, COUT, CIN + 16) / 8
    wide = torch.full((N, H, W, 128), 7.0, dtype=torch.float16, device=DEV)
    with net._pass(net.ws, DEV) as p:
        y = p.pointwise("pw", x, (wt, bias), act=K.ACT_RELU, residual=res)
        assert tuple(y.shape) == (N, H, W, COUT)
        assert torch.equal(y.view(M, COUT), K.gemm(x.view(M, CIN), wt, bias=bias, act=K.ACT_RELU, residual=res.view(M, COUT)))
        y2 = p.pointwise("pw", x, (wt2, bias), a2=a2)
        assert torch.equal(y2.view(M, COUT), K.gemm(x.view(M, CIN), wt2, a2=a2.view(M, 16), bias=bias))
        assert p.pointwise("pw", x, (wt, bias), out2d=wide.view(M, 128)[:, 64:96]) is None
        assert torch.equal(wide[..., 64:96].reshape(M, COUT), K.gemm(x.view(M, CIN), wt, bias=bias))
        assert bool((wide[..., :64] == 7.0).all()) and bool((wide[..., 96:] == 7.0).all())
        f32 = torch.empty((M, COUT), dtype=torch.float32, device=DEV)
        assert p.pointwise("pw", x, (wt, None), out2d=f32, out_f32=True) is None
        assert torch.equal(f32, K.gemm(x.view(M, CIN), wt, out_f32=True))
        for t in (y, y2):
            p.give(t)
    assert net.ws["planned"] and len(net.ws["pool"]) == 2


def test_conv3x3_equals_the_convolution(net):
    from controlanimate_amd import kernels as K
    x, wt, bias = _rnd(7, N, H, W, CIN), _rnd(8, COUT, 3, 3, CIN) / 24, _rnd(9, COUT, dtype=torch.float32)
    ws = net._workspace("conv", lambda dev: {})
    with net._pass(ws, DEV) as p:
        y = p.conv3x3("conv", x, (wt, bias), act=K.ACT_RELU)
        assert tuple(y.shape) == (N, H, W, COUT) and torch.equal(y, K.conv3x3(x, wt, bias=bias, act=K.ACT_RELU))
        y2 = p.conv3x3("conv", x, (wt, bias), stride=2, split_k=False)
        assert tuple(y2.shape) == (N, H // 2, W // 2, COUT) and torch.equal(y2, K.conv3x3(x, wt, bias=bias, stride=2, split_k=False))
        p.give(y), p.give(y2)
    ptrs = [sl[0].data_ptr() for sl in ws["pool"]]
    with net._pass(ws, DEV) as p:       # the second pass gets the same buffers and allocates nothing
        assert p.conv3x3("conv", x, (wt, bias), act=K.ACT_RELU).data_ptr() == y.data_ptr()
        assert p.conv3x3("conv", x, (wt, bias), stride=2, split_k=False).data_ptr() == y2.data_ptr()
    assert [sl[0].data_ptr() for sl in ws["pool"]] == ptrs
