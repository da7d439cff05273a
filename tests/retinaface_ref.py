"""The specification of controlanimate_amd.face_align: the front half of facexlib's FaceRestoreHelper as GFPGANer.enhance drives it --
RetinaFace(network_name='resnet50', phase='test'), its priors, decode and NMS, get_face_landmarks_5's filters, the 5-point fit and
cv2.warpAffine to 512 x 512 -- in numpy and torch on the CPU, fp32 for the network and float64 for everything behind it.

UNPINNED: restated from memory of facexlib's published code (detection/retinaface.py, retinaface_net.py, retinaface_utils.py,
utils/face_restoration_helper.py) and of OpenCV's warpAffine / remap.  facexlib, torchvision and OpenCV are absent here and no
detection_Resnet50_Final.pth is available.  The one pinned part is the body: `body` reproduces transformers' ResNetModel (torchvision's
v1.5 bottleneck arithmetic) on tests/golden/retinaface_body_tiny.npz.

Stated rules (each is what the device is held to):

  slope      facexlib's LeakyReLU slope is 0.1 if the FPN / SSH module's out_channels <= 64 else 0: `leaky_slope`.  At 256 it is 0, a ReLU;
             only slope 0 is built (`network` raises for anything else)
  decode     float64 arithmetic on the fp32 head outputs, every result rounded once to fp32 (facexlib computes in fp32)
  score      1 / (1 + exp(c0 - c1)) in float64, rounded to fp32; kept when the fp32 score > float32(conf_threshold)
  order      score descending, exact ties to the LOWER prior index (facexlib: numpy's unstable argsort()[::-1]; differs on ties only)
  nms        py_cpu_nms on the fp32 boxes, its arithmetic in float64: areas (x2 - x1 + 1)(y2 - y1 + 1), a box stays while its overlap with
             every box kept before it is <= nms_threshold
  eyes       a face is dropped when the distance between landmarks 0 and 1 (float64, sqrt) is below eye_dist_threshold
  choice     only_keep_largest: the first largest (x2 - x1)(y2 - y1); else only_center_face: the first nearest box centre to (W / 2, H / 2)
  fit        DELIBERATE DEVIATION: cv2.estimateAffinePartial2D(method=LMEDS) is a seeded random search with a Levenberg-Marquardt polish and is
             not restated; `similarity_fit` is the closed-form least-squares 4-parameter similarity over all five points, float64
  warp       cv2.warpAffine(img, M, (512, 512)), INTER_LINEAR in OpenCV's fixed point, BORDER_CONSTANT with (135, 133, 132) by channel position
  bgr        False: the reference's way -- it hands an RGB array where facexlib expects BGR, so the detector's mean (104, 117, 123) and the
             border value meet channels 0, 1, 2 of the array as given.  True: the array is reversed on the way in and the crops on the way out
"""
import math

import numpy as np

MIN_SIZES = ((16, 32), (64, 128), (256, 512))
STEPS = (8, 16, 32)
VARIANCE = (0.1, 0.2)
MEAN = (104.0, 117.0, 123.0)
BORDER = (135, 133, 132)
FACE_SIZE = 512
TEMPLATE = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043], [313.08905, 371.15118]], np.float64)
BN_EPS = 1e-5
LAYERS = (3, 4, 6, 3)
MAX_CAND = 1024
OVERFLOW_CAND, OVERFLOW_FACES = 1, 2
SSH_CONVS = ("conv3X3", "conv5X5_1", "conv5X5_2", "conv7X7_2", "conv7x7_3")


def leaky_slope(out_channels: int) -> float:
    return 0.1 if out_channels <= 64 else 0.0


# ---- the network (torch, fp32 unless the state dict is float64) ------------------------------------------------------------------------
def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """(weight, bias) of a bias-free convolution followed by an eval-mode BatchNorm, in the operands' dtype."""
    scale = gamma / (var + eps) ** 0.5
    return w * scale.reshape(-1, *([1] * (w.ndim - 1))), beta - mean * scale


def _conv_bn(sd, x, conv, bn, stride=1, padding=0):
    import torch.nn.functional as F
    y = F.conv2d(x, sd[conv + ".weight"], None, stride, padding)
    return F.batch_norm(y, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, BN_EPS)


def body(sd, x):
    """torchvision's ResNet-50 v1.5 under facexlib's `body.` names: x [n, 3, H, W] (mean already subtracted) -> the outputs of layer2,
    layer3 and layer4.  The stride sits on the 3x3 convolution; the shortcut is a 1x1 convolution of the block's stride plus BatchNorm."""
    import torch.nn.functional as F
    x = F.relu(_conv_bn(sd, x, "body.conv1", "body.bn1", 2, 3))
    x = F.max_pool2d(x, 3, 2, 1)
    taps = []
    for li, blocks in enumerate(LAYERS, start=1):
        for b in range(blocks):
            p = f"body.layer{li}.{b}"
            stride = 2 if (b == 0 and li > 1) else 1
            y = F.relu(_conv_bn(sd, x, p + ".conv1", p + ".bn1"))
            y = F.relu(_conv_bn(sd, y, p + ".conv2", p + ".bn2", stride, 1))
            y = _conv_bn(sd, y, p + ".conv3", p + ".bn3")
            if b == 0:
                x = _conv_bn(sd, x, p + ".downsample.0", p + ".downsample.1", stride)
            x = F.relu(y + x)
        if li > 1:
            taps.append(x)
    return taps


def preprocess(frames_u8, bgr=False, dtype=None):
    """uint8 [n, H, W, 3] -> [n, 3, H, W]: the bytes as floats minus (104, 117, 123) by channel position (after the reversal when bgr)."""
    import torch
    a = np.asarray(frames_u8)
    if bgr:
        a = a[..., ::-1]
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dtype or torch.float32)
    return (x - torch.tensor(MEAN, dtype=x.dtype)).permute(0, 3, 1, 2).contiguous()


def network(sd, frames_u8, bgr=False):
    """-> (class logits [n, P, 2], boxes [n, P, 4], landmarks [n, P, 10]) in the state dict's dtype and on its device, levels concatenated in
    the priors' order.  The softmax over the class pair is `scores`."""
    import torch
    import torch.nn.functional as F
    dt = sd["body.conv1.weight"].dtype
    out_ch = sd["fpn.output1.0.weight"].shape[0]
    if leaky_slope(out_ch) != 0.0:
        raise NotImplementedError(f"out_channels={out_ch}: only the slope-0 LeakyReLU (out_channels > 64) is built")
    x = preprocess(frames_u8, bgr, dt).to(sd["body.conv1.weight"].device)
    t1, t2, t3 = body(sd, x)

    def cbr(x, name, padding=0, act=True):
        y = _conv_bn(sd, x, name + ".0", name + ".1", 1, padding)
        return F.relu(y) if act else y

    o1, o2, o3 = cbr(t1, "fpn.output1"), cbr(t2, "fpn.output2"), cbr(t3, "fpn.output3")
    o2 = cbr(o2 + F.interpolate(o3, size=o2.shape[2:], mode="nearest"), "fpn.merge2", 1)
    o1 = cbr(o1 + F.interpolate(o2, size=o1.shape[2:], mode="nearest"), "fpn.merge1", 1)
    cls, box, ldm = [], [], []
    for k, f in enumerate((o1, o2, o3)):
        s = f"ssh{k + 1}."
        c3 = cbr(f, s + "conv3X3", 1, False)
        c51 = cbr(f, s + "conv5X5_1", 1, True)
        c5 = cbr(c51, s + "conv5X5_2", 1, False)
        c72 = cbr(c51, s + "conv7X7_2", 1, True)
        c7 = cbr(c72, s + "conv7x7_3", 1, False)
        f = F.relu(torch.cat([c3, c5, c7], 1))
        n = f.shape[0]
        for name, width, dst in (("ClassHead", 2, cls), ("BboxHead", 4, box), ("LandmarkHead", 10, ldm)):
            y = F.conv2d(f, sd[f"{name}.{k}.conv1x1.weight"], sd[f"{name}.{k}.conv1x1.bias"])
            dst.append(y.permute(0, 2, 3, 1).reshape(n, -1, width))
    return torch.cat(cls, 1), torch.cat(box, 1), torch.cat(ldm, 1)


# ---- priors, decode -----------------------------------------------------------------------------------------------------------------------
def level_shapes(h: int, w: int):
    return [(-(-h // s), -(-w // s)) for s in STEPS]


def prior_count(h: int, w: int) -> int:
    return sum(2 * a * b for a, b in level_shapes(h, w))


def priors(h: int, w: int) -> np.ndarray:
    """float64 [P, 4] (cx, cy, s / W, s / H): level by level, cells row-major, two priors per cell; no clip."""
    out = []
    for (fh, fw), step, sizes in zip(level_shapes(h, w), STEPS, MIN_SIZES):
        i, j = np.mgrid[0:fh, 0:fw]
        cx, cy = (j + 0.5) * step / w, (i + 0.5) * step / h
        lvl = np.stack([np.stack([cx, cy, np.full(cx.shape, s / w), np.full(cx.shape, s / h)], -1) for s in sizes], 2)   # [fh, fw, 2, 4]
        out.append(lvl.reshape(-1, 4))
    return np.concatenate(out).astype(np.float64)


def scores(cls) -> np.ndarray:
    """fp32 [.., 2] logits -> the face probability, float64 arithmetic, rounded once to fp32."""
    c = np.asarray(cls, np.float32).astype(np.float64)
    return (1.0 / (1.0 + np.exp(c[..., 0] - c[..., 1]))).astype(np.float32)


def decode(box, ldm, pri, h: int, w: int):
    """fp32 boxes [P, 4] and landmarks [P, 10] of one frame -> (corners [P, 4], landmarks [P, 10]) in pixels, fp32."""
    b, l = np.asarray(box, np.float32).astype(np.float64), np.asarray(ldm, np.float32).astype(np.float64)
    cxy = pri[:, :2] + b[:, :2] * VARIANCE[0] * pri[:, 2:]
    wh = pri[:, 2:] * np.exp(b[:, 2:] * VARIANCE[1])
    lo = cxy - wh / 2
    hi = wh + lo
    corners = np.concatenate([lo, hi], 1) * np.array([w, h, w, h], np.float64)
    pts = (pri[:, None, :2] + l.reshape(-1, 5, 2) * VARIANCE[0] * pri[:, None, 2:]) * np.array([w, h], np.float64)
    return corners.astype(np.float32), pts.reshape(-1, 10).astype(np.float32)


def order(score, idx):
    """Positions into idx: score descending, ties to the lower prior index."""
    return np.lexsort((idx, -score.astype(np.float64)))


def iou_plus1(a, b) -> float:
    """py_cpu_nms's overlap of two fp32 boxes, float64."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    ww = max(0.0, min(a[2], b[2]) - max(a[0], b[0]) + 1.0)
    hh = max(0.0, min(a[3], b[3]) - max(a[1], b[1]) + 1.0)
    inter = ww * hh
    return inter / ((a[2] - a[0] + 1.0) * (a[3] - a[1] + 1.0) + (b[2] - b[0] + 1.0) * (b[3] - b[1] + 1.0) - inter)


def nms(boxes, thresh: float):
    """Greedy over boxes already in order -> the kept positions."""
    keep = []
    for i in range(len(boxes)):
        if all(iou_plus1(boxes[k], boxes[i]) <= thresh for k in keep):
            keep.append(i)
    return keep


def detect(cls, box, ldm, h, w, conf_threshold=0.97, nms_threshold=0.4, eye_dist_threshold=5.0, max_faces=4, only_center_face=False,
           only_keep_largest=False, max_cand=MAX_CAND):
    """One frame's fp32 head outputs -> dict(dets fp32 [max_faces, 15] (x1, y1, x2, y2, score, 10 landmark coordinates; zero rows behind
    count), count, overflow, priors: the kept prior indices)."""
    sc = scores(cls)
    idx = np.nonzero(sc > np.float32(conf_threshold))[0]
    overflow = 0
    o = order(sc[idx], idx)
    if len(o) > max_cand:
        overflow |= OVERFLOW_CAND
        o = o[:max_cand]
    idx = idx[o]
    corners, pts = decode(np.asarray(box)[idx], np.asarray(ldm)[idx], priors(h, w)[idx], h, w)
    faces = []
    for k in nms(corners, nms_threshold):
        p = pts[k].astype(np.float64)
        if math.sqrt((p[0] - p[2]) ** 2 + (p[1] - p[3]) ** 2) < eye_dist_threshold:
            continue
        faces.append(k)
    c64 = corners.astype(np.float64)
    if faces and only_keep_largest:
        area = [(c64[k, 2] - c64[k, 0]) * (c64[k, 3] - c64[k, 1]) for k in faces]
        faces = [faces[int(np.argmax(area))]]
    elif faces and only_center_face:
        dist = [math.sqrt(((c64[k, 0] + c64[k, 2]) / 2 - w / 2) ** 2 + ((c64[k, 1] + c64[k, 3]) / 2 - h / 2) ** 2) for k in faces]
        faces = [faces[int(np.argmin(dist))]]
    if len(faces) > max_faces:
        overflow |= OVERFLOW_FACES
        faces = faces[:max_faces]
    dets = np.zeros((max_faces, 15), np.float32)
    for r, k in enumerate(faces):
        dets[r, :4], dets[r, 4], dets[r, 5:] = corners[k], sc[idx[k]], pts[k]
    return {"dets": dets, "count": len(faces), "overflow": overflow, "priors": [int(idx[k]) for k in faces]}


# ---- the fit --------------------------------------------------------------------------------------------------------------------------------
def similarity_fit(src, dst=TEMPLATE) -> np.ndarray:
    """The least-squares u = a x - b y + tx, v = b x + a y + ty over the point pairs, float64 [2, 3] = [[a, -b, tx], [b, a, ty]].  The sums
    run over the points in order, operation by operation as written (the device repeats them)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = len(src)
    mx = my = mu = mv = 0.0
    for i in range(n):
        mx, my, mu, mv = mx + src[i, 0], my + src[i, 1], mu + dst[i, 0], mv + dst[i, 1]
    mx, my, mu, mv = mx / n, my / n, mu / n, mv / n
    sa = sb = ss = 0.0
    for i in range(n):
        x, y, u, v = src[i, 0] - mx, src[i, 1] - my, dst[i, 0] - mu, dst[i, 1] - mv
        sa = sa + (x * u + y * v)
        sb = sb + (x * v - y * u)
        ss = ss + (x * x + y * y)
    a, b = sa / ss, sb / ss
    return np.array([[a, -b, mu - (a * mx - b * my)], [b, a, mv - (b * mx + a * my)]], np.float64)


def invert_affine(m) -> np.ndarray:
    """cv2.invertAffineTransform / the inversion inside cv2.warpAffine, float64, operation by operation."""
    m = np.asarray(m, np.float64)
    d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[1, 1] * d, m[0, 0] * d
    a12, a21 = m[0, 1] * -d, m[1, 0] * -d
    return np.array([[a11, a12, -a11 * m[0, 2] - a12 * m[1, 2]], [a21, a22, -a21 * m[0, 2] - a22 * m[1, 2]]], np.float64)


def inverse_affine(m, upscale_factor=1) -> np.ndarray:
    return invert_affine(m) * float(upscale_factor)


# ---- the warp -------------------------------------------------------------------------------------------------------------------------------
AB_BITS, INTER_BITS = 10, 5
AB_SCALE, INTER_TAB = 1 << AB_BITS, 1 << INTER_BITS
ROUND_DELTA = AB_SCALE // INTER_TAB // 2   # 16
COEF_BITS = 15


def _sat_int(v):
    """saturate_cast<int>(double): cvRound (round half to even), clamped to int32."""
    return np.clip(np.rint(v), -2147483648.0, 2147483647.0).astype(np.int64)


def warp_affine(img, m, size=FACE_SIZE, border=BORDER, bgr=False) -> np.ndarray:
    """cv2.warpAffine(img, m, (size, size)) with its defaults but BORDER_CONSTANT `border`, uint8 [H, W, 3] -> [size, size, 3].

    The matrix is inverted (invert_affine); the source coordinate of destination (x, y) at 10 fractional bits is
    X = sat_int((M[0][1] y + M[0][2]) 1024) + 16 + sat_int(M[0][0] x 1024) (Y likewise with row 1), shifted down to 5 fractional bits;
    sx = sat_short(X >> 5), fx = X & 31.  The four taps (sx, sy), (sx + 1, sy), (sx, sy + 1), (sx + 1, sy + 1) -- the border value where a
    tap lies outside the image -- are weighted by the 15-bit table, which for the bilinear kernel holds exact integers
    (32 - fy)(32 - fx) 32, (32 - fy) fx 32, fy (32 - fx) 32, fy fx 32 (sum 2^15); the result is (sum + 2^14) >> 15."""
    img = np.asarray(img)
    if bgr:
        return warp_affine(img[..., ::-1], m, size, border, False)[..., ::-1]
    h, w, _ = img.shape
    inv = invert_affine(m)
    xs, ys = np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64)
    adelta, bdelta = _sat_int(inv[0, 0] * xs * AB_SCALE), _sat_int(inv[1, 0] * xs * AB_SCALE)
    x0 = _sat_int((inv[0, 1] * ys + inv[0, 2]) * AB_SCALE) + ROUND_DELTA
    y0 = _sat_int((inv[1, 1] * ys + inv[1, 2]) * AB_SCALE) + ROUND_DELTA
    # (int32 wrap-around of the sums, as the C code's int arithmetic gives)
    X = (((x0[:, None] + adelta[None, :]) + 2 ** 31) % 2 ** 32 - 2 ** 31) >> (AB_BITS - INTER_BITS)
    Y = (((y0[:, None] + bdelta[None, :]) + 2 ** 31) % 2 ** 32 - 2 ** 31) >> (AB_BITS - INTER_BITS)
    sx, sy = np.clip(X >> INTER_BITS, -32768, 32767), np.clip(Y >> INTER_BITS, -32768, 32767)
    fx, fy = X & (INTER_TAB - 1), Y & (INTER_TAB - 1)
    bval = np.array(border, np.int64)
    acc = np.zeros((size, size, 3), np.int64)
    for dy, dx, wt in ((0, 0, (32 - fy) * (32 - fx)), (0, 1, (32 - fy) * fx), (1, 0, fy * (32 - fx)), (1, 1, fy * fx)):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        pix = np.where(inside[..., None], img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), bval)
        acc += pix * (wt * 32)[..., None]
    return ((acc + (1 << (COEF_BITS - 1))) >> COEF_BITS).astype(np.uint8)


def align(frame, dets, count, upscale_factor=1, bgr=False):
    """One frame and its detections -> (crops uint8 [count, 512, 512, 3], affine [count, 2, 3], inverse_affine [count, 2, 3])."""
    crops, ms, invs = [], [], []
    for r in range(count):
        m = similarity_fit(np.asarray(dets[r, 5:15], np.float32).astype(np.float64).reshape(5, 2))
        ms.append(m)
        invs.append(inverse_affine(m, upscale_factor))
        crops.append(warp_affine(frame, m, bgr=bgr))
    return (np.stack(crops) if crops else np.zeros((0, FACE_SIZE, FACE_SIZE, 3), np.uint8), np.array(ms).reshape(-1, 2, 3), np.array(invs).reshape(-1, 2, 3))


# ---- seeded weights (tests, tools) ---------------------------------------------------------------------------------------------------------
def seeded_state_dict(key_shapes: dict, seed: int = 0) -> dict:
    """A state dict of the given shapes: He-scaled convolutions, BatchNorm statistics and affine terms away from the trivial, small head
    biases -- activations neither vanish nor grow through the fifty layers."""
    import torch
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in key_shapes.items():
        if k.endswith("running_var"):
            v = 0.6 + 0.8 * torch.rand(shape, generator=g)
        elif k.endswith("running_mean"):
            v = 0.2 * torch.randn(shape, generator=g)
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            v = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif k.endswith("conv1x1.bias"):
            v = 0.1 * torch.randn(shape, generator=g)
        elif k.endswith("weight"):
            v = 0.8 + 0.4 * torch.rand(shape, generator=g)
            if ".bn3." in k:
                v = v * 0.5   # (the residual sum would otherwise double the variance per block)
        else:
            v = 0.2 * torch.randn(shape, generator=g)
        sd[k] = v
    if "body.conv1.weight" in sd:
        sd["body.conv1.weight"] = sd["body.conv1.weight"] / 64.0   # (the input is bytes minus a mean: of the order of 100)
    return sd
