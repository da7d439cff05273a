"""The fixtures that tests/test_face_paste_cpu.py and tests/test_face_paste_gpu.py share: the reduced ParseNet geometry with its seeded weights
and faces (and the fp32 specification's logits for them, computed once), the planted blur masks and the planted paste cases.  Everything is
generated from seeds; nothing is read from disk."""
import functools

import numpy as np
import torch

import facepaste_ref as P

SMALL = dict(in_size=128, base_ch=32, res_depth=2, ch_range=(32, 64))
SEED, CLASS_BIAS = 1, 4.0
# The label test compares where the specification's top-two margin exceeds four times the device's maximum absolute logit error, and at most
# 5 % of the pixels may lie below that margin.  For logits that vary like noise the share below a margin d is about 0.5 d / sigma, and the
# bf16 error is 3 % of sigma, so in bf16 only per-class biases that settle most pixels can meet the condition: (seed, class_bias) per dtype.
# fp16 keeps the fixture of the other tests (ten classes above 1 % of the pixels); bf16 takes stronger biases (two classes above 1 %).
LABEL_CASE = {torch.float16: (SEED, CLASS_BIAS), torch.bfloat16: (17, 6.0)}
# The device's maximum absolute logit error on those fixtures against the fp32 specification: measured on the device by
# test_parsenet_small_logits_and_labels (its docstring has the figures) and recorded here with headroom.  The GPU test holds its own
# measurement to these; the CPU test checks the 5 % condition with them.
LOGIT_ERR = {torch.float16: 0.012, torch.bfloat16: 0.1}


def smooth_faces(n, size, seed=0) -> np.ndarray:
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) * (128.0 / size)
    rng = np.random.default_rng(seed)
    out = np.empty((n, size, size, 3), np.float64)
    for i in range(n):
        for c in range(3):
            out[i, :, :, c] = 127 + 100 * np.sin(0.05 * (i + 1) * xx + 0.07 * (c + 1) * yy + i + seed) + rng.normal(0, 10, (size, size))
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=4)
def small_sd(seed=SEED, class_bias=CLASS_BIAS) -> dict:
    """The seeded reduced-geometry state dict, every tensor rounded to fp16 (what the device packs from)."""
    return {k: v.half().float() for k, v in P.seeded_state_dict(SMALL, seed, class_bias).items()}


@functools.lru_cache(maxsize=1)
def small_faces() -> np.ndarray:
    return smooth_faces(3, SMALL["in_size"], seed=3)


@functools.lru_cache(maxsize=4)
def small_logits(bgr=False, seed=SEED, class_bias=CLASS_BIAS):
    """The fp32 specification's parsing maps [3, 19, 128, 128] for the seeded faces: computed once, never changed."""
    with torch.no_grad():
        return P.logits(small_sd(seed, class_bias), small_faces(), bgr, SMALL)


@functools.lru_cache(maxsize=1)
def blur_masks() -> np.ndarray:
    """uint8 [4, 512, 512]: random blobs, all 0, all 255, a single 255 pixel in a corner."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:512, 0:512]
    blobs = np.zeros((512, 512), bool)
    for _ in range(12):
        cy, cx, ry, rx = rng.integers(0, 512), rng.integers(0, 512), rng.integers(8, 120), rng.integers(8, 120)
        blobs |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
    corner = np.zeros((512, 512), np.uint8)
    corner[0, 511] = 255
    return np.stack([blobs.astype(np.uint8) * 255, np.zeros((512, 512), np.uint8), np.full((512, 512), 255, np.uint8), corner])


@functools.lru_cache(maxsize=1)
def planted_soft_masks() -> np.ndarray:
    """float64 [9, 512, 512] in [0, 1] with full mantissas, zero on the outer 10 rows and columns: what the blur could have written."""
    rng = np.random.default_rng(13)
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float64)
    out = []
    for i in range(9):
        bump = np.exp(-(((yy - 256 - 20 * (i % 3 - 1)) / (150 + 10 * i)) ** 4 + ((xx - 256) / (170 - 8 * i)) ** 4))
        m = np.clip(bump * (0.9 + 0.1 * np.sin(0.03 * xx + 0.05 * yy + i)) + rng.uniform(0, 0.01, (512, 512)), 0, 1)
        m[:10], m[-10:], m[:, :10], m[:, -10:] = 0, 0, 0, 0
        out.append(m)
    return np.stack(out)


@functools.lru_cache(maxsize=8)
def paste_case(hw, f):
    """A window of three frames of hw (the faces were found there) pasted at upscale f, max_faces = 3, counts 0 / 1 / 3.  Frame 2's faces:
    A hangs over the top and left edges, B overlaps A and hangs over the bottom, C hangs over the right edge.  The slots behind a frame's
    count hold NaN matrices and noise: nothing may read them.  -> dict(background [3, h f, w f, 3], restored [9, 512, 512, 3], masks
    [9, 512, 512], inverse [3, 3, 2, 3], count [3])."""
    h, w = hw
    hu, wu = int(h * f), int(w * f)
    rng = np.random.default_rng(100 * h + w + f)
    background = rng.integers(0, 256, (3, hu, wu, 3), dtype=np.uint8)
    restored = np.clip(smooth_faces(9, 512, seed=9).astype(np.int64) + rng.integers(-20, 21, (9, 512, 512, 3)), 0, 255).astype(np.uint8)

    def mat(scale, angle, tx, ty):      # face coordinates -> frame coordinates at the final size
        a, b = scale * np.cos(angle), scale * np.sin(angle)
        return np.array([[a, -b, tx], [b, a, ty]], np.float64)

    s = 0.75 * hu / 512.0
    inverse = np.full((3, 3, 2, 3), np.nan)
    inverse[1, 0] = mat(s * 0.9, 0.15, 0.31 * wu + 0.123, 0.12 * hu + 0.377)
    inverse[2, 0] = mat(s, -0.2, -0.2 * hu + 0.25, -0.05 * hu + 0.61)
    inverse[2, 1] = mat(s, 0.1, 0.18 * wu + 0.5, 0.42 * hu + 0.05)
    inverse[2, 2] = mat(s * 0.8, 0.3, wu - 0.35 * hu + 0.77, 0.2 * hu + 0.19)
    return {"background": background, "restored": restored, "masks": planted_soft_masks(), "inverse": inverse, "count": np.array([0, 1, 3], np.int32)}
