"""Specification of the GFPGAN face restoration the reference runs on every emitted frame when `use_face_enhancer` is set
(modules/upscaler.py:53-70: `GFPGANer(arch='clean', channel_multiplier=2).enhance(...)`): the network `GFPGANv1Clean` with its
`StyleGAN2GeneratorCSFT` decoder, from real `nn` modules under the published parameter names, and the numpy container around it for
aligned faces (`enhance(..., has_aligned=True)`).

UNPINNED: gfpgan, basicsr, facexlib and OpenCV are third-party packages that are absent here, and no GFPGANv1.3.pth is available.
The modules below are a restatement of the published gfpganv1_clean_arch.py / stylegan2_clean_arch.py and of GFPGANer.enhance /
basicsr's img2tensor / tensor2img; key names and parity with them are not checked against the packages or a real weight file.

    encoder   leaky(conv_body_first 1x1) -> log2(out_size) - 2 ResBlock(down) (their outputs are the unet_skips) -> leaky(final_conv)
              -> final_linear over the NCHW flattening of the [256, 4, 4] map -> (2 log2(out_size) - 2) latents of 512
    up path   per level: feat = ResBlock(up)(feat + unet_skips[i]); scale_i, shift_i = condition_scale[i](feat), condition_shift[i](feat)
    decoder   constant -> StyleConv -> ToRGB, then per level StyleConv(upsample) -> SFT on the second half of the channels ->
              StyleConv -> ToRGB(+ bilinear x2 of the previous image); noise is an explicit input (GFPGANer calls the net with
              randomize_noise=True): one map at 4x4, then two per level

Every forward below takes `q`, applied to every activation a narrow-type chain would store (identity for the specification);
`emulate` is the same chain with q = rounding to fp16 / bf16, fp32 accumulation, weights rounded by `round_weights`.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

SQRT2 = 2.0 ** 0.5


def _id(t):
    return t


def unet_channels(channel_multiplier=2, narrow=1):
    un = narrow * 0.5
    return {4: int(512 * un), 8: int(512 * un), 16: int(512 * un), 32: int(512 * un), 64: int(256 * channel_multiplier * un),
            128: int(128 * channel_multiplier * un), 256: int(64 * channel_multiplier * un), 512: int(32 * channel_multiplier * un),
            1024: int(16 * channel_multiplier * un)}


def stylegan_channels(channel_multiplier=2, narrow=1):
    return {4: int(512 * narrow), 8: int(512 * narrow), 16: int(512 * narrow), 32: int(512 * narrow), 64: int(256 * channel_multiplier * narrow),
            128: int(128 * channel_multiplier * narrow), 256: int(64 * channel_multiplier * narrow), 512: int(32 * channel_multiplier * narrow),
            1024: int(16 * channel_multiplier * narrow)}


def resize2(x, up):
    return F.interpolate(x, scale_factor=2 if up else 0.5, mode="bilinear", align_corners=False)


class NormStyleCode(nn.Module):
    def forward(self, x):
        return x * torch.rsqrt(torch.mean(x ** 2, dim=1, keepdim=True) + 1e-8)


class ModulatedConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, num_style_feat, demodulate=True, sample_mode=None, eps=1e-8):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.demodulate, self.sample_mode, self.eps = demodulate, sample_mode, eps
        self.modulation = nn.Linear(num_style_feat, in_channels, bias=True)
        nn.init.constant_(self.modulation.bias, 1.0)
        self.weight = nn.Parameter(torch.randn(1, out_channels, in_channels, kernel_size, kernel_size) / math.sqrt(in_channels * kernel_size ** 2))
        self.padding = kernel_size // 2

    def forward(self, x, style):
        b, c, h, w = x.shape
        style = self.modulation(style).view(b, 1, c, 1, 1)
        weight = self.weight * style
        if self.demodulate:
            demod = torch.rsqrt(weight.pow(2).sum([2, 3, 4]) + self.eps)
            weight = weight * demod.view(b, self.out_channels, 1, 1, 1)
        weight = weight.view(b * self.out_channels, c, self.kernel_size, self.kernel_size)
        if self.sample_mode == "upsample":
            x = resize2(x, True)
        b, c, h, w = x.shape
        out = F.conv2d(x.reshape(1, b * c, h, w), weight, padding=self.padding, groups=b)
        return out.view(b, self.out_channels, *out.shape[2:4])


class StyleConv(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, num_style_feat, demodulate=True, sample_mode=None):
        super().__init__()
        self.modulated_conv = ModulatedConv2d(in_channels, out_channels, kernel_size, num_style_feat, demodulate=demodulate, sample_mode=sample_mode)
        self.weight = nn.Parameter(torch.zeros(1))  # the noise weight
        self.bias = nn.Parameter(torch.zeros(1, out_channels, 1, 1))

    def forward(self, x, style, noise):
        out = self.modulated_conv(x, style) * SQRT2
        out = out + self.weight * noise
        out = out + self.bias
        return F.leaky_relu(out, 0.2)


class ToRGB(nn.Module):
    def __init__(self, in_channels, num_style_feat, upsample=True):
        super().__init__()
        self.upsample = upsample
        self.modulated_conv = ModulatedConv2d(in_channels, 3, 1, num_style_feat, demodulate=False, sample_mode=None)
        self.bias = nn.Parameter(torch.zeros(1, 3, 1, 1))

    def forward(self, x, style, skip=None):
        out = self.modulated_conv(x, style) + self.bias
        if skip is not None:
            if self.upsample:
                skip = resize2(skip, True)
            out = out + skip
        return out


class ConstantInput(nn.Module):
    def __init__(self, num_channel, size):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(1, num_channel, size, size))

    def forward(self, batch):
        return self.weight.repeat(batch, 1, 1, 1)


class StyleGAN2GeneratorCSFT(nn.Module):
    def __init__(self, out_size, num_style_feat=512, num_mlp=8, channel_multiplier=2, narrow=1, sft_half=True):
        super().__init__()
        self.num_style_feat, self.sft_half = num_style_feat, sft_half
        layers = [NormStyleCode()]
        for _ in range(num_mlp):
            layers += [nn.Linear(num_style_feat, num_style_feat, bias=True), nn.LeakyReLU(0.2, inplace=True)]
        self.style_mlp = nn.Sequential(*layers)  # unused with input_is_latent=True
        ch = stylegan_channels(channel_multiplier, narrow)
        self.channels = ch
        self.constant_input = ConstantInput(ch[4], size=4)
        self.style_conv1 = StyleConv(ch[4], ch[4], 3, num_style_feat, demodulate=True, sample_mode=None)
        self.to_rgb1 = ToRGB(ch[4], num_style_feat, upsample=False)
        self.log_size = int(math.log(out_size, 2))
        self.num_layers = (self.log_size - 2) * 2 + 1
        self.num_latent = self.log_size * 2 - 2
        self.style_convs, self.to_rgbs, self.noises = nn.ModuleList(), nn.ModuleList(), nn.Module()
        for layer_idx in range(self.num_layers):
            res = 2 ** ((layer_idx + 5) // 2)
            self.noises.register_buffer(f"noise{layer_idx}", torch.randn(1, 1, res, res))
        cin = ch[4]
        for i in range(3, self.log_size + 1):
            cout = ch[2 ** i]
            self.style_convs.append(StyleConv(cin, cout, 3, num_style_feat, demodulate=True, sample_mode="upsample"))
            self.style_convs.append(StyleConv(cout, cout, 3, num_style_feat, demodulate=True, sample_mode=None))
            self.to_rgbs.append(ToRGB(cout, num_style_feat, upsample=True))
            cin = cout

    def forward(self, latent, conditions, noise, q=_id):
        """latent [n, num_latent, 512]; conditions [scale_0, shift_0, scale_1, ...]; noise: num_layers maps [n, 1, h, w]."""
        out = self.constant_input(latent.shape[0])
        out = q(self.style_conv1(out, latent[:, 0], noise[0]))
        skip = self.to_rgb1(out, latent[:, 1])
        i = 1
        for conv1, conv2, n1, n2, to_rgb in zip(self.style_convs[::2], self.style_convs[1::2], noise[1::2], noise[2::2], self.to_rgbs):
            out = conv1(out, latent[:, i], n1)
            if i < len(conditions):
                if self.sft_half:
                    same, sft = torch.split(out, out.size(1) // 2, dim=1)
                    out = torch.cat([same, sft * conditions[i - 1] + conditions[i]], dim=1)
                else:
                    out = out * conditions[i - 1] + conditions[i]
            out = q(out)
            out = q(conv2(out, latent[:, i + 1], n2))
            skip = to_rgb(out, latent[:, i + 2], skip)
            i += 2
        return skip


class ResBlock(nn.Module):
    def __init__(self, in_channels, out_channels, mode="down"):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, in_channels, 3, 1, 1)
        self.conv2 = nn.Conv2d(in_channels, out_channels, 3, 1, 1)
        self.skip = nn.Conv2d(in_channels, out_channels, 1, bias=False)
        self.up = mode == "up"

    def forward(self, x, q=_id):
        out = q(F.leaky_relu(self.conv1(x), 0.2))
        out = q(resize2(out, self.up))
        out = q(F.leaky_relu(self.conv2(out), 0.2))
        x = q(resize2(x, self.up))
        return q(out + self.skip(x))


class GFPGANv1Clean(nn.Module):
    def __init__(self, out_size, num_style_feat=512, channel_multiplier=2, narrow=1, different_w=True, input_is_latent=True, sft_half=True):
        super().__init__()
        assert different_w and input_is_latent and sft_half, "the reference's configuration (GFPGANer arch='clean')"
        self.num_style_feat = num_style_feat
        ch = unet_channels(channel_multiplier, narrow)
        self.log_size = int(math.log(out_size, 2))
        first = 2 ** self.log_size
        self.conv_body_first = nn.Conv2d(3, ch[first], 1)
        cin = ch[first]
        self.conv_body_down = nn.ModuleList()
        for i in range(self.log_size, 2, -1):
            self.conv_body_down.append(ResBlock(cin, ch[2 ** (i - 1)], mode="down"))
            cin = ch[2 ** (i - 1)]
        self.final_conv = nn.Conv2d(cin, ch[4], 3, 1, 1)
        cin = ch[4]
        self.conv_body_up = nn.ModuleList()
        for i in range(3, self.log_size + 1):
            self.conv_body_up.append(ResBlock(cin, ch[2 ** i], mode="up"))
            cin = ch[2 ** i]
        self.toRGB = nn.ModuleList([nn.Conv2d(ch[2 ** i], 3, 1) for i in range(3, self.log_size + 1)])  # unused on this path
        self.final_linear = nn.Linear(ch[4] * 4 * 4, (self.log_size * 2 - 2) * num_style_feat)
        self.stylegan_decoder = StyleGAN2GeneratorCSFT(out_size, num_style_feat, 8, channel_multiplier, narrow, sft_half)
        self.condition_scale, self.condition_shift = nn.ModuleList(), nn.ModuleList()
        for i in range(3, self.log_size + 1):
            c = ch[2 ** i]
            self.condition_scale.append(nn.Sequential(nn.Conv2d(c, c, 3, 1, 1), nn.LeakyReLU(0.2, True), nn.Conv2d(c, c, 3, 1, 1)))
            self.condition_shift.append(nn.Sequential(nn.Conv2d(c, c, 3, 1, 1), nn.LeakyReLU(0.2, True), nn.Conv2d(c, c, 3, 1, 1)))

    def encode(self, x, q=_id):
        """-> (latent [n, num_latent, 512] fp32, conditions)."""
        feat = q(F.leaky_relu(self.conv_body_first(x), 0.2))
        skips = []
        for blk in self.conv_body_down:
            feat = blk(feat, q)
            skips.insert(0, feat)
        feat = q(F.leaky_relu(self.final_conv(feat), 0.2))
        latent = self.final_linear(feat.reshape(feat.size(0), -1)).view(feat.size(0), -1, self.num_style_feat)
        conditions = []
        for i, blk in enumerate(self.conv_body_up):
            feat = blk(q(feat + skips[i]), q)
            for branch in (self.condition_scale[i], self.condition_shift[i]):
                conditions.append(q(branch[2](q(F.leaky_relu(branch[0](feat), 0.2)))))
        return latent, conditions

    def forward(self, x, noise, q=_id):
        """x [n, 3, S, S] in [-1, 1]; noise: the decoder's maps [n, 1, h, w] (or [n, h, w]) -> the image [n, 3, S, S] before the clamp."""
        noise = [t if t.dim() == 4 else t[:, None] for t in noise]
        assert len(noise) == self.stylegan_decoder.num_layers
        latent, conditions = self.encode(x, q)
        return self.stylegan_decoder(latent, conditions, noise, q)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
def make_net(out_size, seed):
    """A seeded network whose activations keep their scale through the depth (He-scaled convolutions), with NON-ZERO noise weights and
    StyleConv / ToRGB biases (the published initial value 0 would leave those paths untested)."""
    torch.manual_seed(seed)
    net = GFPGANv1Clean(out_size).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("modulated_conv.weight") or "modulation" in name or "constant_input" in name:
                continue
            if name.startswith("stylegan_decoder.") and name.endswith(".weight") and p.numel() == 1:
                p.copy_(torch.rand(1, generator=g) * 0.2 + 0.1)
            elif name.endswith(".bias"):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)
            elif name.startswith("final_linear"):
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p.shape[1]) ** 0.5)
            elif p.dim() == 4:
                # LeakyReLU(0.2) keeps 0.52 of a unit variance: gain 1.9 restores it; a ResBlock adds two paths of half the variance each;
                # the last convolution of an SFT branch is small, around scale = 1 (its bias, below) and shift = 0
                fan = p.shape[1] * p.shape[2] * p.shape[3]
                gain = 0.5 if name.endswith("skip.weight") else (1.0 if name.endswith("conv2.weight") else (0.05 if name.startswith("condition_") and ".2." in name else 1.9))
                p.copy_(torch.randn(p.shape, generator=g) * (gain / fan) ** 0.5)
        for branch in net.condition_scale:
            branch[2].bias.add_(1.0)
        for m in net.modules():
            if isinstance(m, ModulatedConv2d):
                m.modulation.weight.copy_(torch.randn(m.modulation.weight.shape, generator=g) * (0.25 / 512 ** 0.5))
                m.modulation.bias.fill_(1.0)
        for t in [net.stylegan_decoder.to_rgb1, *net.stylegan_decoder.to_rgbs]:  # the image is the sum of one term per level
            t.modulated_conv.weight.mul_(0.3)
    return net


def round_weights(sd, dtype):
    """The state dict with every tensor of two or more dimensions rounded to `dtype` (kept float32): what a narrow-type chain holds."""
    return {k: (v.to(dtype).float() if v.dim() >= 2 and v.is_floating_point() else v.clone()) for k, v in sd.items()}


def make_noises(out_size, n, seed):
    g = torch.Generator().manual_seed(seed)
    log = int(math.log(out_size, 2))
    return [torch.randn(n, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2), generator=g) for i in range((log - 2) * 2 + 1)]


def make_faces(out_size, n, seed):
    """uint8 [n, S, S, 3]: smooth structure plus noise, covering 0 .. 255."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, 8, 8, generator=g)
    img = F.interpolate(low, size=(out_size, out_size), mode="bilinear", align_corners=False) + 0.15 * torch.randn(n, 3, out_size, out_size, generator=g)
    return (img.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ---- the container: GFPGANer.enhance(img, has_aligned=True) ---------------------------------------------------------------------
def container_in(faces_u8, reverse_channels=True):
    """uint8 [n, S, S, 3] -> the net's input [n, 3, S, S]: img / 255 (float32), the channel order reversed (enhance takes BGR and
    img2tensor(bgr2rgb=True) swaps; the reference hands it RGB), normalize(0.5, 0.5)."""
    a = np.asarray(faces_u8).astype(np.float32) / np.float32(255.0)
    if reverse_channels:
        a = a[..., ::-1]
    a = (a - np.float32(0.5)) / np.float32(0.5)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))


def container_out(image, reverse_channels=True):
    """The net's output [n, 3, S, S] (any float type) -> uint8 [n, S, S, 3]: tensor2img(rgb2bgr=True, min_max=(-1, 1)): clamp, (x + 1) / 2,
    * 255, numpy .round() (half to even), uint8."""
    a = np.asarray(image.detach().cpu().float().numpy(), dtype=np.float32)
    a = np.clip(a, -1.0, 1.0)
    a = (a - np.float32(-1.0)) / np.float32(2.0)
    a = a.transpose(0, 2, 3, 1)
    if reverse_channels:
        a = a[..., ::-1]
    return (a * np.float32(255.0)).round().astype(np.uint8)


def pre_round64(image, reverse_channels=True):
    """float64 value in front of the rounding, in the layout of container_out."""
    a = image.detach().cpu().double().numpy().clip(-1.0, 1.0)
    a = ((a + 1.0) / 2.0 * 255.0).transpose(0, 2, 3, 1)
    return a[..., ::-1] if reverse_channels else a


def restore_aligned(net, faces_u8, noises, reverse_channels=True):
    with torch.no_grad():
        return container_out(net(container_in(faces_u8, reverse_channels), noises), reverse_channels)


def emulate(net, faces_u8, noises, dtype, reverse_channels=True):
    """The pre-clamp image [n, 3, S, S] of the chain with every stored activation rounded to `dtype` (fp32 accumulation; latents, styles
    and the RGB image stay fp32).  `net` holds weights already rounded by round_weights."""
    def q(t):
        return t.to(dtype).float()
    with torch.no_grad():
        return net(container_in(faces_u8, reverse_channels), noises, q)


# ---- the identity the device path rests on -----------------------------------------------------------------------------------------
def factored_modconv(x, style_s, weight, demodulate=True, upsample=False, eps=1e-8, scaled=False):
    """modconv(x, style) = demod[n, o] * conv(W, s[n, i] * x), demod = rsqrt(sum_i s^2 Wsq[o, i] + eps), Wsq = sum_k W^2; with
    `scaled`, s is divided by its per-image largest magnitude m and demod' = rsqrt(sum (s / m)^2 Wsq + eps / m^2) = m * demod.
    x [n, ci, h, w], style_s [n, ci] (after the modulation Linear), weight [co, ci, k, k]."""
    wsq = weight.pow(2).sum([2, 3])
    s = style_s
    e = torch.full((s.shape[0], 1), eps, dtype=s.dtype)
    if scaled:
        m = s.abs().amax(dim=1, keepdim=True)
        s, e = s / m, e / (m * m)
    if upsample:
        x = resize2(x, True)
    out = F.conv2d(x * s[:, :, None, None], weight, padding=weight.shape[-1] // 2)
    if demodulate:
        out = out * torch.rsqrt((s * s) @ wsq.t() + e)[:, :, None, None]
    elif scaled:
        out = out * m[:, :, None, None]
    return out


# ---- fixtures of the stage tests -----------------------------------------------------------------------------------------------------
BAND = 1e-3  # a float64 pre-round value closer than this to a half-integer may round either way in fp32


def make_finish_fixture(seed, n=2, size=48):
    """float32 [n, 3, size, size] for the finish kernel: values over -1.4 .. 1.4 (a fifth clamped), and a row of special ones: the ends, 0,
    values next to the ends, a NaN-free set of exact level centres and of near-ties."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, 3, size, size, generator=g) * 2.8 - 1.4)
    levels = torch.arange(size, dtype=torch.float32)
    x[0, 0, 0] = levels * 5 / 255.0 * 2 - 1          # level centres
    x[0, 1, 0] = (levels * 5 + 0.5) / 255.0 * 2 - 1    # next to ties: inside the band
    x[0, 2, 0, :6] = torch.tensor([-1.0, 1.0, 0.0, -1.0000001, 1.0000001, -0.99999994])
    return x


def in_band(pre64):
    """Where the float64 value in front of the rounding lies within BAND of a half-integer."""
    return np.abs(pre64 - np.floor(pre64) - 0.5) < BAND


def resample_ref(x_nhwc, up, dtype):
    """The bilinear resize by 2 or 1/2 of an NHWC tensor of `dtype`: fp32 torch interpolate (align_corners=False), rounded to `dtype`."""
    y = resize2(x_nhwc.float().permute(0, 3, 1, 2).contiguous(), up)
    return y.permute(0, 2, 3, 1).contiguous().to(dtype)


class FakeHelper:
    """Records its calls; crops fixed windows of the frame and pastes the restored ones back."""

    def __init__(self, size, corners):
        self.size, self.corners, self.calls = size, corners, []
        self.cropped_faces, self.restored_faces, self.img = [], [], None

    def clean_all(self):
        self.calls.append("clean_all")
        self.cropped_faces, self.restored_faces, self.img = [], [], None

    def read_image(self, img):
        self.calls.append("read_image")
        self.img = np.asarray(img)

    def get_face_landmarks_5(self, only_center_face=False, eye_dist_threshold=None):
        self.calls.append(("get_face_landmarks_5", only_center_face, eye_dist_threshold))
        return len(self.corners)

    def align_warp_face(self):
        self.calls.append("align_warp_face")
        self.cropped_faces = [self.img[y:y + self.size, x:x + self.size].copy() for y, x in self.corners]

    def add_restored_face(self, face):
        self.calls.append("add_restored_face")
        self.restored_faces.append(face)

    def get_inverse_affine(self, path):
        self.calls.append(("get_inverse_affine", path))

    def paste_faces_to_input_image(self, upsample_img=None):
        self.calls.append(("paste_faces_to_input_image", upsample_img is not None))
        out = (self.img if upsample_img is None else np.asarray(upsample_img)).copy()
        k = out.shape[0] // self.img.shape[0]
        for (y, x), f in zip(self.corners, self.restored_faces):
            out[y * k:y * k + self.size, x * k:x * k + self.size] = f
        return out
