"""CPU: the nearest-x2 upsampling convolution as four 2x2 phase convolutions (layers.phase_weights, ca_conv_up2_phase).

The identity: conv3x3(nearest_x2(x), w, padding=1) at output pixel (2y + py, 2x + px) reads only the source pixels
(y + py - 1 + dy, x + px - 1 + dx), dy, dx in {0, 1}; the nine taps that land on the same source pixel are summed into
wp[2 py + px][:, dy, dx, :].  A source pixel outside the image is the zero padding of the upsampled image, so borders need no
special weights -- checked down to a 1x1 source image, where every tap but one is padding.  Also pins which shapes
`ca_conv_up2_phase_supported` takes by default (no launch: the answer is a pure function of the arguments).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F


def phase_sum(x: torch.Tensor, wp: torch.Tensor) -> torch.Tensor:
    """The four-phase form spelled out in torch: x [N, Cin, H, W], wp [4, Cout, 2, 2, Cin] -> [N, Cout, 2H, 2W]."""
    n, cin, h, w = x.shape
    cout = wp.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))  # source pixel (-1 .. H, -1 .. W)
    y = x.new_zeros(n, cout, 2 * h, 2 * w)
    for py in range(2):
        for px in range(2):
            acc = x.new_zeros(n, cout, h, w)
            for dy in range(2):
                for dx in range(2):
                    src = xp[:, :, py + dy:py + dy + h, px + dx:px + dx + w]  # source (y + py - 1 + dy, x + px - 1 + dx)
                    acc = acc + torch.einsum("nchw,oc->nohw", src, wp[2 * py + px, :, dy, dx, :])
            y[:, :, py::2, px::2] = acc
    return y


@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 8, 12, 5, 7), (1, 4, 4, 1, 1), (3, 4, 6, 1, 3), (1, 4, 6, 3, 1), (1, 16, 8, 8, 8), (2, 4, 4, 2, 2)])
def test_phase_weights_equal_upsample_then_conv(n, cin, cout, h, w):
    from controlanimate_amd.layers import phase_weights
    g = torch.Generator().manual_seed(h * 100 + w)
    wt = torch.randn(cout, cin, 3, 3, generator=g)
    x = torch.randn(n, cin, h, w, generator=g)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, padding=1)
    wp = phase_weights(wt)
    assert wp.shape == (4, cout, 2, 2, cin) and wp.dtype == torch.float32
    got = phase_sum(x, wp)
    err = float((got - want).abs().max()) / float(want.abs().max())
    assert err <= 1e-5, err


def test_phase_weights_tap_table():
    """Rows: py = 0 -> {w[0], w[1] + w[2]}, py = 1 -> {w[0] + w[1], w[2]}; columns alike."""
    from controlanimate_amd.layers import phase_weights
    wt = torch.arange(9, dtype=torch.float32).reshape(1, 1, 3, 3) + 1.0  # [[1,2,3],[4,5,6],[7,8,9]]
    wp = phase_weights(wt)[:, 0, :, :, 0]
    assert wp[0].tolist() == [[1.0, 2 + 3.0], [4 + 7.0, 5 + 6 + 8 + 9.0]]
    assert wp[1].tolist() == [[1 + 2.0, 3.0], [4 + 5 + 7 + 8.0, 6 + 9.0]]
    assert wp[2].tolist() == [[1 + 4.0, 2 + 3 + 5 + 6.0], [7.0, 8 + 9.0]]
    assert wp[3].tolist() == [[1 + 2 + 4 + 5.0, 3 + 6.0], [7 + 8.0, 9.0]]
    assert float(wp.sum()) == 4 * 45.0  # every phase carries all nine taps


def test_only_upsampler_convolutions_pack_phase_weights():
    """A resnet convolution must not grow: only the convolution an Upsample3D owns asks for the phase weights."""
    from controlanimate_amd.resnet import InflatedConv3d, ResnetBlock3D, Upsample3D
    assert Upsample3D(640).conv.up2_phase is True
    assert InflatedConv3d(640, 640).up2_phase is False
    blk = ResnetBlock3D(in_channels=640, out_channels=640, temb_channels=1280)
    assert blk.conv1.up2_phase is False and blk.conv2.up2_phase is False


FAKE = 0x10000  # never dereferenced: the answer only looks at sizes, flags and which pointers are set


@pytest.fixture(scope="module")
def capi():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return _capi


def up2_args(capi, n_img, side, ci, co, **kw):
    a = capi.ConvArgs(x=FAKE, w=FAKE, y=FAKE, images=n_img, hin=side, win=side, cin1=ci, cin2=0, cout=co, stride=1, upsample=1, alpha=1.0,
                      post_scale=1.0, dtype=capi.CA_F16, rows_per_group=0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_supported_rule(capi):
    lib = capi.lib()

    def sup(*a, **kw):
        return lib.ca_conv_up2_phase_supported(C.byref(up2_args(capi, *a, **kw)))

    def name(*a, **kw):
        buf = C.create_string_buffer(64)
        rc = lib.ca_conv_up2_phase_plan_name(C.byref(up2_args(capi, *a, **kw)), buf, 64)
        return buf.value.decode() if rc == 0 else None

    # the three upsamplers of a config-2 step (32 images): 32x32 -> 64x64 at 640 channels is 4 x 128 x 2 = 1024 tiles, 16x16 -> 32x32 at 1280
    # is 4 x 32 x 4 = 512 (two whole rounds of 256); 8x8 -> 16x16 is 128 tiles, half the chip: declined, it stays on the Winograd form
    assert sup(32, 32, 640, 640) == 1
    assert sup(32, 16, 1280, 1280) == 1
    assert sup(32, 8, 1280, 1280) == 0
    assert sup(32, 16, 1280, 1280, dtype=capi.CA_BF16) == 1 and sup(32, 16, 1280, 1280, residual=FAKE, ld_res=1280) == 1
    assert sup(16, 16, 1280, 1280) == 1      # 256 tiles: one whole round
    assert sup(24, 16, 1280, 1280) == 0      # 384 tiles = 1.5 rounds
    # what the kernel does not implement, whatever the size: the kernel's name is not available either
    for kw in (dict(cin1=1280 + 32), dict(cout=1280 + 64), dict(x2=FAKE, cin2=64), dict(out_f32=1), dict(stride=2), dict(upsample=0), dict(pad_asym=1),
               dict(rowbias=FAKE, rows_per_group=1024, ld_rowbias=1280), dict(act=1), dict(post_scale=0.5), dict(dtype=2), dict(x=FAKE + 8),
               dict(residual=FAKE, ld_res=1284), dict(x_is_wino_v=1)):
        assert sup(32, 16, 1280, 1280, **kw) == 0, kw
        assert name(32, 16, 1280, 1280, **kw) is None, kw
    assert sup(2048, 64, 64, 320) == 0       # 2^23 source pixels: past the gather's packed row state
    # implemented but declined for its size: the entry point still runs it (tests reach the kernel at small shapes)
    assert sup(1, 8, 320, 320) == 0 and name(1, 8, 320, 320) == "up2_pq256x320"
    assert name(32, 32, 640, 640) == "up2_pq256x320"


def test_old_entry_points_do_not_move(capi):
    """ca_conv3x3 keeps answering for the upsample case exactly what it answered before the phase form existed."""
    buf = C.create_string_buffer(64)
    for (images, h, cin, cout), want in (((32, 32, 640, 640), "128x128"), ((32, 16, 1280, 1280), "128x128")):
        a = up2_args(capi, images, h, cin, cout, rows_per_group=1, workspace=FAKE, workspace_bytes=1 << 40)
        assert capi.lib().ca_conv3x3_plan_name(C.byref(a), buf, 64) == 0 and buf.value.decode() == want
    a = up2_args(capi, 32, 16, 1280, 1280, rows_per_group=1, workspace=FAKE, workspace_bytes=1 << 40, w_wino=FAKE)
    assert capi.lib().ca_conv3x3_plan_name(C.byref(a), buf, 64) == 0 and buf.value.decode() == "wino_pq256x320"
    assert capi.lib().ca_conv3x3_workspace_bytes(C.byref(a)) == 16 * 8192 * (1280 + 1280) * 2
