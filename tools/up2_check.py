"""The upsampling convolutions of a config-2 step: ca_conv3x3(upsample=1) -- the direct 128x128 kernel or the Winograd form, whichever
the library takes -- beside ca_conv_up2_phase (four 2x2 phase convolutions in one launch of the 256 x 320 kernel), product library.

    python tools/up2_check.py --check          # both forms against fp32 torch at the step's sizes, and against each other
    python tools/up2_check.py --time [ROUNDS]  # same process, interleaved: ROUNDS (default 8) rounds of 5 launches of each form

--time prints one line per shape: median / min / max over the rounds of the per-launch time (device events around 5 launches), the
executed TFLOP/s of the phase form (4 taps) and what ca_conv_up2_phase_supported answers for the shape."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from controlanimate_amd import kernels as K
from controlanimate_amd.layers import phase_weights

DEV = "cuda"
# (images, source side, cin, cout): the three Upsample3D of the UNet at 16 frames 512x512, CFG batch 2; then two sizes around the rule
STEP_SHAPES = [(32, 32, 640, 640), (32, 16, 1280, 1280), (32, 8, 1280, 1280)]
RULE_SHAPES = [(16, 16, 1280, 1280), (16, 32, 640, 640), (24, 16, 1280, 1280), (64, 8, 1280, 1280)]
G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])


def make(images, side, cin, cout, dt=torch.float16, seed=0):
    g = torch.Generator().manual_seed(seed)
    w32 = torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5
    d = dict(x=torch.randn(images, side, side, cin, generator=g).to(dt).to(DEV), w32=w32.to(DEV), bias=torch.randn(cout, generator=g).to(DEV) * 0.1,
             w=w32.permute(0, 2, 3, 1).contiguous().to(dt).to(DEV), wp=phase_weights(w32).to(dt).to(DEV), u=None)
    if cin >= 640 and cin % 64 == 0 and cout % 320 == 0:  # (what HipConv3x3.pack stores)
        d["u"] = torch.einsum("xk,oikl,yl->xyoi", G, w32.cpu(), G).reshape(16, cout, cin).contiguous().to(dt).to(DEV)
    return d


def old(d):
    return K.conv3x3(d["x"], d["w"], bias=d["bias"], upsample=True, w_wino=d["u"])


def new(d):
    return K.conv_up2_phase(d["x"], d["wp"], bias=d["bias"])


def label(fn, d):
    K._plan_sink = lab = []
    try:
        fn(d)
    finally:
        K._plan_sink = None
    return lab[-1]


def run5(fn, d):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(5):
        fn(d)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / 5 * 1e3  # us per launch


def check():
    for shape in STEP_SHAPES:
        d = make(*shape)
        ref = F.conv2d(F.interpolate(d["x"].float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest"), d["w32"], bias=d["bias"], padding=1).permute(0, 2, 3, 1)
        yo, yn = old(d), new(d)
        ro, rn = ((yo.float() - ref).norm() / ref.norm()).item(), ((yn.float() - ref).norm() / ref.norm()).item()
        print(f"{shape}: rel-L2 vs fp32 torch: {label(old, d)} {ro:.3e}, {label(new, d)} {rn:.3e}; new vs old {((yn.float() - yo.float()).norm() / ref.norm()).item():.3e}; "
              f"bit-identical repeat: {torch.equal(yn, new(d))}", flush=True)
        assert rn < 2e-3 and torch.isfinite(yn.float()).all()


def time_all(rounds):
    for shape in STEP_SHAPES + RULE_SHAPES:
        images, side, cin, cout = shape
        d = make(*shape)
        for fn in (old, new):
            for _ in range(3):
                fn(d)
        torch.cuda.synchronize()
        to, tn = [], []
        for _ in range(rounds):  # interleaved
            to.append(run5(old, d))
            tn.append(run5(new, d))
        to.sort(), tn.sort()
        flops4 = 2.0 * images * side * side * 4 * cout * 4 * cin
        sup = K.conv_up2_phase_supported(d["x"], d["wp"], bias=d["bias"])
        print(f"{images} x {side}x{side}->{2 * side}x{2 * side} {cin}->{cout}: {label(old, d)} {to[len(to) // 2]:.1f} us [{to[0]:.1f} .. {to[-1]:.1f}] | "
              f"{label(new, d)} {tn[len(tn) // 2]:.1f} us [{tn[0]:.1f} .. {tn[-1]:.1f}] = {flops4 / tn[len(tn) // 2] * 1e-6:.0f} TFLOP/s executed | supported = {int(sup)} "
              f"({rounds} rounds x 5 launches each, interleaved)", flush=True)


if __name__ == "__main__":
    if "--check" in sys.argv:
        check()
    if "--time" in sys.argv:
        i = sys.argv.index("--time")
        time_all(int(sys.argv[i + 1]) if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit() else 8)
