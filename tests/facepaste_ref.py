"""The specification of controlanimate_amd.face_paste: the back half of facexlib's FaceRestoreHelper as GFPGANer.enhance(paste_back=True)
drives it -- ParseNet on every restored face, the parsing mask's colour map, two Gaussian blurs, the inverse warp and the blend -- in torch
on the CPU for the network (fp32) and numpy float64 for everything behind it.

UNPINNED: restated from memory of facexlib's published code (parsing/parsenet.py, utils/face_restoration_helper.py:
paste_faces_to_input_image with use_parse=True) and of OpenCV's GaussianBlur, warpAffine and remap.  facexlib and OpenCV are absent here and
no parsing_parsenet.pth is available, so neither the key names nor a single output byte is checked against them.

Stated rules (each is what the device is held to; "unsure" marks what memory does not settle):

  network    ParseNet(in_size, out_size = in_size, min_feat_size 32, base_ch, parsing_ch 19, res_depth, LeakyReLU(0.2), BatchNorm, ch_range).
             ConvLayer = [nearest x2] -> ReflectionPad2d(1) -> Conv2d(3, stride 2 when 'down', bias unless BatchNorm follows) -> [BatchNorm]
             -> [LeakyReLU(0.2)].  ResidualBlock = shortcut(x) + conv2(conv1(x)); conv1 carries the 'up' scale, BatchNorm and the activation,
             conv2 the 'down' scale and BatchNorm without activation; the shortcut is the identity for scale 'none' at cin == cout, else a
             ConvLayer of the block's scale with bias, no norm, no activation.  out = out_mask_conv(decoder(feat + body(feat))).
             out_img_conv's keys are accepted and never run.  Key names (unsure): encoder.0.conv2d, {encoder, body, decoder}.N.{conv1,
             conv2}.{conv2d, norm.norm}, .shortcut_func.conv2d, out_mask_conv.conv2d, out_img_conv.conv2d
  input      face / 255, channels reversed (img2tensor(bgr2rgb=True)), (x - 0.5) / 0.5 -- each in fp32.  bgr=False is the reference's way: it
             hands RGB where facexlib expects BGR, so the reversal gives the net BGR; bgr=True: the array is turned to BGR first, so the two
             reversals cancel and the net sees the array as given
  labels     argmax over the 19 maps, the lowest index on a tie; mask = MASK_COLORMAP[label] as float64
  blur       cv2.GaussianBlur(mask, (101, 101), 11) twice.  101 taps exp(-x^2 / (2 * 11^2)) normalised to sum 1 in double (getGaussianKernel);
             BORDER_REFLECT_101; the row pass, then the column pass; the SUMMATION ORDER fixed here (unsure what OpenCV's vector code does):
             acc = k0 * x0, then for i = 1 .. 50 in that order acc = acc + k_i * (x_-i + x_+i), every product and sum rounded by itself
  border     the outer 10 rows and columns are zeroed after the second blur, then / 255
  warps      cv2.warpAffine(restored, inverse_affine, (w_up, h_up)): the matrix is inverted (retinaface_ref.invert_affine) and the source
             coordinate computed in OpenCV's fixed point, as retinaface_ref.warp_affine restates it, with border 0 and an arbitrary
             destination size.  The mask takes flags=3 (unsure: taken as the bilinear path on a double image): the same coordinates at 5
             fractional bits, the float table's weights (32 - fy)(32 - fx) / 1024 ... (exact), four products summed in double in the order
             (0, 0), (0, 1), (1, 0), (1, 1), border 0
  offset     when upscale_factor > 1, 0.5 * upscale_factor is added to the translation column of the inverse affine, once
  blend      img = m * inv_restored + (1 - m) * img in float64, carried from face to face; astype(uint8) after the last face
  background upsample_img or the frame, cv2.resize(INTER_LANCZOS4) to (w_up, h_up) = (int(w f), int(h f)); at equal size a copy (the resize
             itself is controlanimate_amd.upscaler's restatement and is not repeated here: `paste` takes a background of the final size)
"""
import math

import numpy as np

import retinaface_ref as R

MASK_COLORMAP = np.array([0, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 0, 255, 0, 0, 0], np.uint8)
PARSING_CH = 19
MIN_FEAT = 32
BN_EPS = 1e-5
FACE_SIZE = 512
BLUR_KSIZE, BLUR_SIGMA, BLUR_EDGE = 101, 11.0, 10
FULL = dict(in_size=512, base_ch=64, res_depth=10, ch_range=(32, 256))


# ---- the network's shape --------------------------------------------------------------------------------------------------------------------
def blocks_of(in_size=512, base_ch=64, res_depth=10, ch_range=(32, 256)):
    """[(name, cin, cout, scale)] of the residual blocks in order: encoder.1 .., body.0 .., decoder.0 ..; widths clipped to ch_range."""
    lo, hi = ch_range
    clip = lambda c: max(lo, min(hi, c))   # noqa: E731
    steps = int(round(math.log2(in_size // MIN_FEAT)))
    out, head = [], base_ch
    for i in range(steps):
        out.append((f"encoder.{i + 1}", clip(head), clip(head * 2), "down"))
        head *= 2
    for i in range(res_depth):
        out.append((f"body.{i}", clip(head), clip(head), "none"))
    for i in range(steps):
        out.append((f"decoder.{i}", clip(head), clip(head // 2), "up"))
        head //= 2
    return out


def head_channels(in_size=512, base_ch=64, res_depth=10, ch_range=(32, 256)) -> int:
    return blocks_of(in_size, base_ch, res_depth, ch_range)[-1][2]


def has_shortcut(cin, cout, scale) -> bool:
    return not (scale == "none" and cin == cout)


def _bn(prefix, c):
    return {f"{prefix}.weight": (c,), f"{prefix}.bias": (c,), f"{prefix}.running_mean": (c,), f"{prefix}.running_var": (c,)}


def key_shapes(in_size=512, base_ch=64, res_depth=10, ch_range=(32, 256), with_img_conv=False) -> dict:
    out = {"encoder.0.conv2d.weight": (base_ch, 3, 3, 3), "encoder.0.conv2d.bias": (base_ch,)}
    for name, cin, cout, scale in blocks_of(in_size, base_ch, res_depth, ch_range):
        if has_shortcut(cin, cout, scale):
            out[f"{name}.shortcut_func.conv2d.weight"], out[f"{name}.shortcut_func.conv2d.bias"] = (cout, cin, 3, 3), (cout,)
        out[f"{name}.conv1.conv2d.weight"] = (cout, cin, 3, 3)
        out.update(_bn(f"{name}.conv1.norm.norm", cout))
        out[f"{name}.conv2.conv2d.weight"] = (cout, cout, 3, 3)
        out.update(_bn(f"{name}.conv2.norm.norm", cout))
    c = head_channels(in_size, base_ch, res_depth, ch_range)
    out["out_mask_conv.conv2d.weight"], out["out_mask_conv.conv2d.bias"] = (PARSING_CH, c, 3, 3), (PARSING_CH,)
    if with_img_conv:
        out["out_img_conv.conv2d.weight"], out["out_img_conv.conv2d.bias"] = (3, c, 3, 3), (3,)
    return out


def seeded_state_dict(geometry=FULL, seed=0, class_bias=2.0, with_img_conv=False) -> dict:
    """Variance-keeping convolutions (2 / fan_in behind the LeakyReLU, i.e. conv2; 1 / fan_in elsewhere: those inputs are not activated),
    BatchNorm statistics away from the trivial, the second BatchNorm of a block at 0.3 of its weight (the residual sum would otherwise
    double the variance per block) and seeded per-class biases of spread `class_bias` on the last layer, so that most pixels have a clear
    winner."""
    import torch
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in key_shapes(with_img_conv=with_img_conv, **geometry).items():
        if k.endswith("running_var"):
            v = 0.6 + 0.8 * torch.rand(shape, generator=g)
        elif k.endswith("running_mean"):
            v = 0.2 * torch.randn(shape, generator=g)
        elif len(shape) == 4:
            v = torch.randn(shape, generator=g) * ((2.0 if ".conv2." in k else 1.0) / (shape[1] * 9)) ** 0.5
        elif k.endswith("norm.norm.weight"):
            v = (0.8 + 0.4 * torch.rand(shape, generator=g)) * (0.3 if ".conv2." in k else 1.0)
        elif k == "out_mask_conv.conv2d.bias":
            v = class_bias * torch.randn(shape, generator=g)
        else:
            v = 0.2 * torch.randn(shape, generator=g)
        sd[k] = v
    return sd


# ---- the network (torch; fp32 unless the state dict is float64) ------------------------------------------------------------------------------
def conv_layer(sd, x, name, scale="none", norm=False, leaky=False):
    import torch.nn.functional as F
    if scale == "up":
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    x = F.pad(x, (1, 1, 1, 1), mode="reflect")
    x = F.conv2d(x, sd[name + ".conv2d.weight"], sd.get(name + ".conv2d.bias"), 2 if scale == "down" else 1)
    if norm:
        p = name + ".norm.norm"
        x = F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, BN_EPS)
    return F.leaky_relu(x, 0.2) if leaky else x


def res_block(sd, x, name, cin, cout, scale):
    idn = conv_layer(sd, x, name + ".shortcut_func", scale) if has_shortcut(cin, cout, scale) else x
    y = conv_layer(sd, x, name + ".conv1", "up" if scale == "up" else "none", True, True)
    y = conv_layer(sd, y, name + ".conv2", "down" if scale == "down" else "none", True, False)
    return idn + y


def preprocess(faces_u8, bgr=False, dtype=None):
    """uint8 [n, S, S, 3] -> [n, 3, S, S]: ((x / 255) - 0.5) / 0.5 in fp32, the channels reversed unless bgr."""
    import torch
    a = np.asarray(faces_u8)
    if not bgr:
        a = a[..., ::-1]
    x = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32)
    x = ((x / 255.0) - 0.5) / 0.5
    return x.permute(0, 3, 1, 2).contiguous().to(dtype or torch.float32)


def logits(sd, faces_u8, bgr=False, geometry=FULL):
    """-> the 19 parsing maps [n, 19, S, S] in the state dict's dtype and on its device."""
    w0 = sd["encoder.0.conv2d.weight"]
    x = preprocess(faces_u8, bgr, w0.dtype).to(w0.device)
    x = conv_layer(sd, x, "encoder.0")
    blocks = blocks_of(**geometry)
    enc = [b for b in blocks if b[0].startswith("encoder")]
    body = [b for b in blocks if b[0].startswith("body")]
    dec = [b for b in blocks if b[0].startswith("decoder")]
    for b in enc:
        x = res_block(sd, x, *b)
    feat = x
    for b in body:
        x = res_block(sd, x, *b)
    x = feat + x
    for b in dec:
        x = res_block(sd, x, *b)
    return conv_layer(sd, x, "out_mask_conv")


def labels_of(lg) -> np.ndarray:
    """[n, 19, S, S] -> uint8 [n, S, S]: the first maximum."""
    a = lg.detach().cpu().numpy() if hasattr(lg, "detach") else np.asarray(lg)
    return np.argmax(a, axis=1).astype(np.uint8)   # (numpy's argmax returns the first maximum)


def top2_margin(lg) -> np.ndarray:
    a = lg.detach().cpu().numpy() if hasattr(lg, "detach") else np.asarray(lg)
    s = np.sort(a.astype(np.float64), axis=1)
    return s[:, -1] - s[:, -2]


# ---- the blur --------------------------------------------------------------------------------------------------------------------------------
def gaussian_taps(ksize=BLUR_KSIZE, sigma=BLUR_SIGMA) -> np.ndarray:
    """cv2.getGaussianKernel(ksize, sigma) in float64: exp(-x^2 / (2 sigma^2)) over x = -(k - 1) / 2 .., divided by their sum (summed in
    index order)."""
    r = (ksize - 1) // 2
    e = np.array([math.exp(-(i - r) * (i - r) / (2.0 * sigma * sigma)) for i in range(ksize)], np.float64)
    s = 0.0
    for v in e:
        s += v
    return e * (1.0 / s)


def half_taps() -> np.ndarray:
    """The centre tap and the 50 behind it (the kernel is symmetric): what the device takes."""
    k = gaussian_taps()
    return np.ascontiguousarray(k[(BLUR_KSIZE - 1) // 2:])


def blur_axis(a, axis, k=None) -> np.ndarray:
    """One 1-D pass along `axis` of a float64 array, BORDER_REFLECT_101, in the fixed order: k0 x0, then + k_i (x_-i + x_+i) for i = 1 .. 50."""
    k = half_taps() if k is None else k
    r = len(k) - 1
    a = np.moveaxis(np.asarray(a, np.float64), axis, -1)
    n = a.shape[-1]
    p = np.pad(a, [(0, 0)] * (a.ndim - 1) + [(r, r)], mode="reflect")   # numpy's 'reflect' is REFLECT_101
    acc = k[0] * p[..., r:r + n]
    for i in range(1, r + 1):
        acc = acc + k[i] * (p[..., r - i:r - i + n] + p[..., r + i:r + i + n])
    return np.moveaxis(acc, -1, axis)


def gaussian_blur(a) -> np.ndarray:
    """cv2.GaussianBlur(a, (101, 101), 11) of [.., H, W]: the row pass (along x), then the column pass."""
    return blur_axis(blur_axis(a, -1), -2)


def soft_mask(mask_u8, zero_border=True) -> np.ndarray:
    """uint8 0 / 255 mask [.., 512, 512] -> float64: blurred twice, the outer 10 rows and columns zeroed, / 255."""
    m = gaussian_blur(gaussian_blur(np.asarray(mask_u8).astype(np.float64)))
    if zero_border:
        t = BLUR_EDGE
        m[..., :t, :] = 0
        m[..., -t:, :] = 0
        m[..., :, :t] = 0
        m[..., :, -t:] = 0
    return m / 255.0


# ---- the warps and the blend --------------------------------------------------------------------------------------------------------------
def _coords(m, h_out, w_out):
    """cv2.warpAffine's source coordinates for an h_out x w_out destination: (sx, sy, fx, fy), 5 fractional bits."""
    inv = R.invert_affine(m)
    xs, ys = np.arange(w_out, dtype=np.float64), np.arange(h_out, dtype=np.float64)
    adelta, bdelta = R._sat_int(inv[0, 0] * xs * R.AB_SCALE), R._sat_int(inv[1, 0] * xs * R.AB_SCALE)
    x0 = R._sat_int((inv[0, 1] * ys + inv[0, 2]) * R.AB_SCALE) + R.ROUND_DELTA
    y0 = R._sat_int((inv[1, 1] * ys + inv[1, 2]) * R.AB_SCALE) + R.ROUND_DELTA
    X = (((x0[:, None] + adelta[None, :]) + 2 ** 31) % 2 ** 32 - 2 ** 31) >> (R.AB_BITS - R.INTER_BITS)
    Y = (((y0[:, None] + bdelta[None, :]) + 2 ** 31) % 2 ** 32 - 2 ** 31) >> (R.AB_BITS - R.INTER_BITS)
    sx, sy = np.clip(X >> R.INTER_BITS, -32768, 32767), np.clip(Y >> R.INTER_BITS, -32768, 32767)
    return sx, sy, X & (R.INTER_TAB - 1), Y & (R.INTER_TAB - 1)


_TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))


def _tap_weights(fx, fy):
    return [(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx]


def warp_u8(img, m, h_out, w_out) -> np.ndarray:
    """cv2.warpAffine(uint8 [H, W, 3], m, (w_out, h_out)): fixed-point bilinear, border 0."""
    img = np.asarray(img)
    h, w, _ = img.shape
    sx, sy, fx, fy = _coords(m, h_out, w_out)
    acc = np.zeros((h_out, w_out, 3), np.int64)
    for (dy, dx), wt in zip(_TAPS, _tap_weights(fx, fy)):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        pix = np.where(inside[..., None], img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), 0)
        acc += pix * (wt * 32)[..., None]
    return ((acc + (1 << (R.COEF_BITS - 1))) >> R.COEF_BITS).astype(np.uint8)


def warp_f64(img, m, h_out, w_out) -> np.ndarray:
    """cv2.warpAffine(float64 [H, W], m, (w_out, h_out), flags=3) taken as the bilinear path: float table weights, summed in double."""
    img = np.asarray(img, np.float64)
    h, w = img.shape
    sx, sy, fx, fy = _coords(m, h_out, w_out)
    acc = None
    for (dy, dx), wt in zip(_TAPS, _tap_weights(fx, fy)):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        pix = np.where(inside, img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0.0)
        prod = pix * (wt.astype(np.float32) * np.float32(1.0 / 1024.0)).astype(np.float64)
        acc = prod if acc is None else acc + prod
    return acc


def paste(background, restored, masks, inverse_affines, upscale_factor=1) -> np.ndarray:
    """One frame: background uint8 [h_up, w_up, 3] (already at the final size), restored uint8 [count, 512, 512, 3], masks float64
    [count, 512, 512] (soft_mask's), inverse_affines float64 [count, 2, 3] -> uint8 [h_up, w_up, 3]."""
    bg = np.asarray(background)
    h_up, w_up, _ = bg.shape
    img = bg.astype(np.float64)
    touched = False
    for face, mask, inv in zip(restored, masks, inverse_affines):
        m = np.array(inv, np.float64, copy=True)
        if upscale_factor > 1:
            m[:, 2] += 0.5 * upscale_factor
        v = warp_u8(face, m, h_up, w_up).astype(np.float64)
        s = warp_f64(mask, m, h_up, w_up)[:, :, None]
        img = s * v + (1 - s) * img
        touched = True
    return img.astype(np.uint8) if touched else bg.copy()
