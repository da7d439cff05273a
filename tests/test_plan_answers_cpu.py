"""CPU: every answer of the GEMM / convolution launch planner (csrc/ca_gemm_plan.h), pinned over a sweep of sizes and flags.

`tests/golden/plan_answers.txt` holds one line per argument set: what `ca_gemm_plan_name` (return code, label), `ca_gemm_workspace_bytes`,
`ca_gemm_row_sums_parts`, `ca_gemm_ln_inline_supported` and `ca_gemm_wants_finished_stats` say about a dense launch, and what
`ca_conv3x3_plan_name`, `ca_conv3x3_workspace_bytes`, `ca_conv_up2_phase_supported` and `ca_conv_up2_phase_plan_name` (return code) say
about a convolution.  Arguments the library rejects are lines too (negative return code, label "-").  The file was written by
`table()` below running against a library built from the commit BEFORE the planner was gathered into one header, so it is the record
of what the scattered copies answered; this test rebuilds the table from the current library and compares line by line.  A change of
a threshold in the planner changes lines here on purpose: re-record with `PYTHONPATH=. python tests/test_plan_answers_cpu.py > tests/golden/plan_answers.txt`
and review the diff -- tests/test_dispatch_plan.py says which of the moved shapes belong to the benchmark workload.

Line formats (flags joined with "+", "-" for none; kept short: the file has to stay below 256 KB):
    d M N K flags rc label workspace_bytes row_sums_parts ln_inline_supported wants_finished_stats
    c images H W cin cout flags w|n rc label workspace_bytes up2_supported up2_plan_name_rc       (w: a workspace is offered, n: none)
Flags: res = residual, ws = workspace offered, ln=s / ln=i / ln=P = folded LayerNorm with finished statistics / in-kernel statistics / P
partial sums, k2=h / k2=32 = a second source of K / 2 / 32 channels, rb=G = row bias in groups of G rows, g = GEGLU, f = fragment-ordered
weights, rs = row sums asked for, f32 = fp32 output; s2 = stride 2, up = nearest-x2 upsample, c2=h = second source of Cin / 2 channels,
wino = Winograd weights offered, pad = asymmetric padding, bf16.
"""
import ctypes as C
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_answers.txt")
FAKE = 0x10000  # never dereferenced: the plan only looks at sizes, flags and which pointers are set

# the ten flag sets of test_dispatch_plan.py::test_every_plan_is_a_kernel_that_exists ...
DENSE_FLAGS = [dict(), dict(res=True), dict(ws=True), dict(ln="s"), dict(ln=2), dict(k2="h"), dict(rb=4096), dict(g=True),
               dict(g=True, ln="s", ws=True), dict(ln="i", f=True, ws=True),
               # ... and: row sums, partial LayerNorm sums with and without scratch, the fragment-ordered weights alone and with row-bias groups
               # that are / are not whole 128-row tiles, fp32 output, a second source that leaves K1 no multiple of 64
               dict(rs=True), dict(rs=True, res=True), dict(ln=1), dict(ln=1, ws=True), dict(ln=4), dict(ln=4, ws=True),
               dict(f=True), dict(f=True, rb=4032), dict(f=True, rb=4096), dict(f32=True), dict(k2=32)]
DENSE_M = (32, 2048, 8192, 32768, 131072, 1 << 23)
DENSE_N = (4, 64, 320, 960, 1280, 5120, 10240)
DENSE_K = (8, 64, 320, 1280, 5120)

# that test's convolution flag sets (its workspace=False set is the "n" half of every set here) and: the Winograd weights offered,
# asymmetric padding, bf16, fp32 output
CONV_FLAGS = [dict(), dict(s2=True), dict(up=True), dict(c2="h"), dict(wino=True), dict(pad=True), dict(bf16=True), dict(f32=True)]
CONV_IMAGES = (1, 32)
CONV_H = (3, 8, 32, 64, 128)
CONV_CH = ((8, 320), (320, 4), (320, 320), (640, 320), (1280, 1280), (2560, 1280))


def _flags(kw):
    return "+".join(k if v is True else f"{k}={v}" for k, v in kw.items()) or "-"


def dense_line(capi, m, n, k, kw):
    lib = capi.lib()
    k2 = kw.get("k2", 0)
    k2 = k // 2 if k2 == "h" else k2
    geglu, ln = int(kw.get("g", 0)), kw.get("ln")
    a = capi.GemmArgs(a=FAKE, w=FAKE, c=FAKE, m=m, n=n, k1=k - k2, k2=k2, lda=k - k2, lda2=k2, ldc=n // 2 if geglu else n,
                      alpha=1.0, post_scale=1.0, dtype=capi.CA_F16, geglu=geglu, rows_per_group=1, out_f32=int(kw.get("f32", 0)))
    if k2:
        a.a2 = FAKE
    if kw.get("res"):
        a.residual, a.ld_res = FAKE, n
    if ln == "i":
        a.ln_colsum, a.ln_eps = FAKE, 1e-5
    elif ln == "s":
        a.ln_colsum, a.ln_stats, a.ln_eps = FAKE, FAKE, 1e-5
    elif ln is not None:
        a.ln_colsum, a.ln_stats, a.ln_eps, a.ln_parts = FAKE, FAKE, 1e-5, ln
    if kw.get("rs"):
        a.row_sums_out = FAKE
    if kw.get("ws"):
        a.workspace, a.workspace_bytes = FAKE, 1 << 40
    if kw.get("f"):
        a.w_frag = FAKE
    if kw.get("rb"):
        a.rowbias, a.rows_per_group, a.ld_rowbias = FAKE, kw["rb"], n
    buf = C.create_string_buffer(64)
    rc = lib.ca_gemm_plan_name(C.byref(a), buf, 64)
    label = buf.value.decode() if rc == 0 else "-"
    nums = (lib.ca_gemm_workspace_bytes(C.byref(a)), lib.ca_gemm_row_sums_parts(C.byref(a)), lib.ca_gemm_ln_inline_supported(C.byref(a)),
            lib.ca_gemm_wants_finished_stats(C.byref(a)))
    return f"d {m} {n} {k} {_flags(kw)} {rc} {label} " + " ".join(str(int(v)) for v in nums)


def conv_line(capi, images, h, w, cin, cout, kw, workspace):
    lib = capi.lib()
    cin2 = cin // 2 if kw.get("c2") == "h" and cin > 8 else 0
    a = capi.ConvArgs(x=FAKE, w=FAKE, y=FAKE, images=images, hin=h, win=w, cin1=cin - cin2, cin2=cin2, cout=cout, stride=2 if kw.get("s2") else 1,
                      upsample=int(kw.get("up", 0)), alpha=1.0, post_scale=1.0, dtype=capi.CA_BF16 if kw.get("bf16") else capi.CA_F16,
                      rows_per_group=1, pad_asym=int(kw.get("pad", 0)), out_f32=int(kw.get("f32", 0)))
    if cin2:
        a.x2 = FAKE
    if kw.get("wino"):
        a.w_wino = FAKE
    if workspace:
        a.workspace, a.workspace_bytes = FAKE, 1 << 40
    buf = C.create_string_buffer(64)
    rc = lib.ca_conv3x3_plan_name(C.byref(a), buf, 64)
    label = buf.value.decode() if rc == 0 else "-"
    nums = (lib.ca_conv3x3_workspace_bytes(C.byref(a)), lib.ca_conv_up2_phase_supported(C.byref(a)),
            lib.ca_conv_up2_phase_plan_name(C.byref(a), C.create_string_buffer(64), 64))
    return f"c {images} {h} {w} {cin} {cout} {_flags(kw)} {'w' if workspace else 'n'} {rc} {label} " + " ".join(str(int(v)) for v in nums)


def table(capi):
    lines = [dense_line(capi, m, n, k, kw) for m in DENSE_M for n in DENSE_N for k in DENSE_K for kw in DENSE_FLAGS]
    for images in CONV_IMAGES:
        for h in CONV_H:
            for w in (h, 3 * h // 2) if h % 2 == 0 else (h,):  # rectangular where 3H / 2 is even
                lines += [conv_line(capi, images, h, w, cin, cout, kw, ws) for cin, cout in CONV_CH for kw in CONV_FLAGS for ws in (True, False)]
    return lines


@pytest.fixture(scope="module")
def current():
    from controlanimate_amd import _build, _capi
    _build.build(verbose=False)
    return table(_capi)


def test_fixture_is_not_vacuous():
    """What was checked on the recording side: most kernels are reached, and every numeric query answers both zero and non-zero."""
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert os.path.getsize(GOLDEN) <= 256 * 1024
    fields = [line.split() for line in want]
    assert all(len(f) == (11 if f[0] == "d" else 13) for f in fields)
    rc_label = [(f[5], f[6]) if f[0] == "d" else (f[8], f[9]) for f in fields]
    labels = {label for rc, label in rc_label if rc == "0"}
    assert len(labels) >= 12, sorted(labels)
    assert any(int(rc) < 0 for rc, _ in rc_label)  # rejected arguments are recorded, not skipped
    for kind, col in (("d", 7), ("d", 8), ("d", 9), ("d", 10), ("c", 10), ("c", 11)):
        vals = {int(f[col]) for f in fields if f[0] == kind}
        assert 0 in vals and any(v > 0 for v in vals), (kind, col)


def test_every_planner_answer_is_the_recorded_one(current):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(current) == len(want), (len(current), len(want))
    diff = [(i + 1, w, c) for i, (w, c) in enumerate(zip(want, current)) if w != c]
    assert not diff, f"{len(diff)} of {len(want)} lines differ (line, recorded, now); the first: {diff[:5]}"


if __name__ == "__main__":
    from controlanimate_amd import _capi
    print("\n".join(table(_capi)))
