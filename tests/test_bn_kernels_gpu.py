"""The training-mode BatchNorm kernels of rein48_amd/csrc/r48_bn.hip and r48_bn_finish.h, each C-ABI entry
against the float64 references of tests/update_refs.py (bn_forward, bn_backward and their _from_sums
forms, held to torch's batch_norm + autograd by test_update_kernels_host.py), at small and ragged row
counts, with and without the ReLU mask, and from records of sums the test makes itself.

Conventions (test_update_kernels_gpu.py's): every output is a slice of a poisoned buffer whose guard is
checked, inputs are compared with their originals after the call, every entry is checked, and each
test prints its worst error / bound ratio. u = 2^-24 is fp32's unit roundoff; a bound is a count of
fp32 roundings times the magnitudes involved (fwd_bounds, bwd_bounds and the docstrings). Nothing here
is a tolerance measured on the device.

Geometry: a thread owns 8 channels of a row, so a block step covers RPB = 256 / (C / 8) rows (64, 32,
16 for C = 32, 64, 128); a reduce block takes 4 RPB rows (4 loads in flight per thread) and the reduce
grid caps at 1,024 blocks. SMALL row counts: 1, 2, RPB - 1, RPB, RPB + 1, 4 RPB - 1, 4 RPB (every thread
in the unrolled loop), 4 RPB + 1, 20 RPB + 1 (some threads unrolled, the others up to 4 times in the
tail loop); BIG: 4096 RPB (the cap exactly) and 4096 RPB + RPB + 1 (a second grid-stride pass, ragged;
more than 256 records for the finish).

Planted channels (bn_case; rows >= 2): constant; |mean| / std = 128 across a binade boundary with row
0 at the mean; the two values 1 and 1 + 2^-7; zero but for the LAST row; gamma = 0; gamma < 0; and in
the backward a channel whose mask bits are all 0 (whose y is <= 0).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import update_refs as U
from test_ntuple_gpu import guard_ok, guarded
from test_update_kernels_gpu import DEV, bits, check, dev, host, lib, ptr, report, stream, worst

pytestmark = pytest.mark.gpu
u = U.U
F32 = np.float32
D53 = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -20      # on every bound: the float64 roundings of the finish and the terms of order u^2
CONST, FAR, TWO, LAST, G0, GNEG = 1, 9, 10, 18, 19, 27       # planted channels (two per channel group of 8)
CHANNELS = [32, 64, 128]
MOM_EPS = [(0.1, 1e-5), (0.0, 1e-3), (1.0, 1e-5), (0.1, 1e-3), (0.0, 1e-5), (1.0, 1e-3)]


def rpb(ch):
    return 256 // (ch // 8)


def reduce_blocks(rows, ch):
    return min(1024, max(1, -(-rows // (4 * rpb(ch)))))


def chain(rows, ch):
    """The most rows one thread of a reduce kernel adds up."""
    return -(-rows // (reduce_blocks(rows, ch) * rpb(ch)))


def small_rows(ch):
    r = rpb(ch)
    return [1, 2, r - 1, r, r + 1, 4 * r - 1, 4 * r, 4 * r + 1, 20 * r + 1]


def big_rows(ch):
    r = rpb(ch)
    return [4096 * r, 4096 * r + r + 1]


SMALL = [(ch, rows) for ch in CHANNELS for rows in small_rows(ch)]
BIG = [(ch, rows) for ch in CHANNELS for rows in big_rows(ch)]


def f32(v):
    return float(F32(v))


def bf16_tensor(t):
    return t.to(torch.bfloat16)


def f64(t):
    """A bf16 tensor's values as float64 numpy."""
    return t.double().cpu().numpy()


def bf16_bits(t):
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def bn_case(rows, ch, seed):
    """bf16 x, res, dy, y [rows, ch] (CPU tensors), random mask bytes [rows, ch / 8], fp32 gamma, beta,
    rm, rv [ch]. x is N(mu_c, sd_c^2) per channel, |mu_c| up to a few sd_c, with the planted channels
    of the module docstring; dy and y are N(0, 1) with +-0 sprinkled in; the last channel of the mask
    is all 0 and its y is <= 0.
    The |mean| / std = 128 channel sits at 1.004: bf16 leaves such a channel a handful of values, whose
    squares have 16 bits, so fp32 sums them exactly until a sum needs more than 24 bits. Just above 1
    (values on both sides, the lower ones on the 2^-8 grid) the plain sum of squares of a 256-row block
    (C = 32) does, and sums without the row-0 shift lose what the bound of the shifted sums excludes."""
    gen = torch.Generator().manual_seed(seed)
    mu, sd = torch.randn(ch, generator=gen) * 2, torch.rand(ch, generator=gen) + 0.5
    mu[FAR], sd[FAR] = 1.004, 1.004 / 128
    x = torch.randn(rows, ch, generator=gen) * sd + mu
    if rows >= 2:
        x[:, CONST] = -2.75
        x[0, FAR] = 1.004
        x[:, TWO] = torch.where(torch.rand(rows, generator=gen) < 0.5, 1.0, 1.0 + 2.0 ** -7)
        x[0, TWO], x[1, TWO] = 1.0, 1.0 + 2.0 ** -7
        x[:, LAST] = 0.0
        x[rows - 1, LAST] = 3.0
    res, dy, y = (torch.randn(rows, ch, generator=gen) for _ in range(3))
    zero = torch.rand(rows, ch, generator=gen)
    for t in (dy, y):
        t[zero < 0.05] = 0.0
        t[zero > 0.95] = -0.0
    y[:, ch - 1] = -y[:, ch - 1].abs()
    mask = torch.randint(0, 256, (rows, ch // 8), generator=gen, dtype=torch.uint8)
    mask[:, ch // 8 - 1] &= 0x7F
    gamma = torch.randn(ch, generator=gen) * 0.5 + 1.0
    gamma[G0], gamma[GNEG] = 0.0, -1.25
    beta, rm, rv = torch.randn(ch, generator=gen), torch.randn(ch, generator=gen), torch.rand(ch, generator=gen) + 0.5
    return {"rows": rows, "C": ch, "x": bf16_tensor(x), "res": bf16_tensor(res), "dy": bf16_tensor(dy),
            "y": bf16_tensor(y), "mask": mask, "gamma": gamma.numpy(), "beta": beta.numpy(), "rm": rm.numpy(),
            "rv": rv.numpy()}


def mask_bits(mask, ch):
    """uint8 [rows, ch / 8] -> bool [rows, ch]: bit k of byte j is channel 8 j + k."""
    return np.unpackbits(mask, axis=1, bitorder="little").astype(bool).reshape(mask.shape[0], ch)


# ------------------------------------------------------------------------------------ the bounds
def inv_err(var, e_var, eps):
    """The most 1 / sqrt(var + eps) moves when var moves by e_var and stays >= 0 (the kernel clamps)."""
    inv = 1.0 / np.sqrt(var + eps)
    return np.maximum(1.0 / np.sqrt(np.maximum(var - e_var, 0.0) + eps) - inv, inv - 1.0 / np.sqrt(var + e_var + eps))


def fwd_bounds(f, n, e_dm, e_var, gamma, eps, momentum):
    """f: update_refs.bn_forward / bn_from_sums; e_dm, e_var: the error of the kernel's mean and biased
    variance before their cast. Each output is one float64 expression of those, cast to fp32 once
    (u |value|): mean: e_dm; invstd: inv_err; a = gamma invstd: |gamma| inv_err; b = beta - mean a:
    |a| e_dm + |mean| |gamma| inv_err (+ their product); running mean: momentum e_dm; running variance:
    momentum (n / (n - 1)) e_var."""
    e_inv = inv_err(f["var"], e_var, eps)
    g = np.abs(gamma)
    e = {"mean": e_dm + u * np.abs(f["mean"]), "invstd": e_inv + u * f["invstd"], "a": g * e_inv + u * np.abs(f["a"]),
         "b": np.abs(f["a"]) * e_dm + np.abs(f["mean"]) * g * e_inv + e_dm * g * e_inv + u * np.abs(f["b"])}
    if f["rm"] is not None:
        e["rm"] = momentum * e_dm + u * np.abs(f["rm"])
        e["rv"] = momentum * (n / (n - 1.0) if n > 1 else 1.0) * e_var + u * np.abs(f["rv"])
    return {k: v * SLACK for k, v in e.items()}


def fwd_direct_bounds(f, x0, rows, ch, gamma, eps, momentum):
    """r48_bn_forward's own statistics pass. K = chain + 10 roundings reach an addend of a block's
    record: d = x - x0 (one; twice in d^2), the thread's chain of adds (fused for d^2), at most 4
    shuffle levels, 3 adds over the waves, and 1 spare; the records are summed in float64. So the shifted
    sums err by K u sum |x - x0| and K u sum (x - x0)^2, and var = S2 / n - dm^2 by K u S2mag / n +
    2 |dm| e_dm + e_dm^2 + 4 2^-53 (S2mag / n + dm^2) (the float64 cancellation)."""
    k = chain(rows, ch) + 10
    dm = f["mean"] - x0
    e_dm = k * u * f["s1_mag"] / rows
    e_var = k * u * f["s2_mag"] / rows + 2 * np.abs(dm) * e_dm + e_dm ** 2 + 4 * D53 * (f["s2_mag"] / rows + dm ** 2)
    return fwd_bounds(f, rows, e_dm, e_var, gamma, eps, momentum)


def merge(top, r, prefix=""):
    """The worst ratio of each output so far."""
    for k, v in r.items():
        top[prefix + k] = max(top.get(prefix + k, 0.0), v)
    return top


def report_all(name, top):
    """One line with every output's worst error / bound ratio (the bf16 outputs y and dx sit near 1
    whenever an entry is close to a rounding tie; the fp32 outputs show the slack of the derived bounds)."""
    print("%s: worst error / bound: %s" % (name, ", ".join("%s %.3g" % kv for kv in top.items())))
    assert all(v <= 1 for v in top.values())


def out_bound(want, e32):
    """A bf16 output whose fp32 value is within e32 of want: half a bf16 ulp of the value it rounds."""
    return U.bf16_half_ulp(np.abs(want) + e32) + e32


def y_ratio(got, f, e, x):
    """y = bf16(relu?(fma(a, x, b) (+ res))): the errors of a and b, one fp32 rounding for the fma and
    one for the add (2 u z_mag covers both), ReLU (1-Lipschitz), then the bf16 rounding."""
    e32 = (e["a"] * np.abs(x) + e["b"] + 2 * u * f["z_mag"]) * SLACK
    return worst(np.abs(got - f["y"]), out_bound(f["y"], e32))


def bwd_bounds(b, rows, ch, mean, invstd, e_sg, e_sgx, save_exact):
    """b: update_refs.bn_backward / _from_sums; e_sg, e_sgx: the errors of the kernel's two sums before
    the finish. save_exact: the reference took the fp32 save as its mean and invstd (the record
    forms); otherwise it took the float64 statistics and the kernel their fp32 roundings, which adds
    u |mean| sum |g| to sgx and one u per use of invstd. All in float64 from there, one cast each:
      dbeta = sg: e_sg + u |dbeta|.   dgamma = invstd sgx: invstd e_sgx + (1 or 2) u |dgamma|.
      a = gamma invstd: (1 or 2) u |a|.   cc = -a invstd dgamma / n: |a| invstd e_dgamma / n + (1 or 4) u |cc|.
      d = -a sg / n - cc mean: |a| e_sg / n + |mean| e_cc + u |d| + (0 or 2) u (|a sg / n| + |cc mean|),
        and the float64 cancellation 4 2^-53 (|a sg / n| + |cc mean|)."""
    n, s = float(rows), 0 if save_exact else 1
    e_dg = invstd * e_sgx + s * u * np.abs(b["dgamma"])
    t1, t2 = np.abs(b["a"] * b["dbeta"]) / n, np.abs(b["cc"] * mean)
    e_cc = np.abs(b["a"]) * invstd * e_dg / n + 3 * s * u * np.abs(b["cc"])
    e = {"dbeta": e_sg + u * np.abs(b["dbeta"]), "dgamma": e_dg + u * np.abs(b["dgamma"]),
         "a": (1 + s) * u * np.abs(b["a"]), "cc": e_cc + u * np.abs(b["cc"]),
         "d": np.abs(b["a"]) * e_sg / n + np.abs(mean) * e_cc + u * np.abs(b["d"]) + (2 * s * u + 4 * D53) * (t1 + t2)}
    return {k: v * SLACK for k, v in e.items()}


def bwd_direct_bounds(b, rows, ch, mean, invstd):
    """r48_bn_backward's own reduction: chain + 8 roundings reach an addend of sum g (the chain, 4
    shuffle levels, 3 wave adds, 1 spare), one more for x - mean in sum g (x - mean); the fp32 mean of
    save is off by u |mean|."""
    k = chain(rows, ch) + 8
    return bwd_bounds(b, rows, ch, mean, invstd, k * u * b["g_mag"],
                      (k + 1) * u * b["gx_mag"] + u * np.abs(mean) * b["g_mag"], False)


def dx_ratio(got, want, b, e, g, x):
    """dx = bf16(fma(a, g, fma(cc, x, d))): the coefficients' errors, two fp32 roundings (2 u of the
    magnitudes covers both), then the bf16 rounding."""
    mag = np.abs(b["a"] * g) + np.abs(b["cc"] * x) + np.abs(b["d"])
    e32 = (e["a"] * np.abs(g) + e["cc"] * np.abs(x) + e["d"] + 2 * u * mag) * SLACK
    return worst(np.abs(got - want), out_bound(want, e32))


# ------------------------------------------------------------------------------------- the calls
class Device:
    """A case's inputs on the device, with the copies that show they were left alone."""

    def __init__(self, case):
        self.case = case
        self.t = {k: dev(v.numpy() if k == "mask" else v.view(torch.int16).numpy()) for k, v in case.items()
                  if k in ("x", "res", "dy", "y", "mask")}
        self.t.update({k: dev(case[k]) for k in ("gamma", "beta")})
        self.keep = {k: v.clone() for k, v in self.t.items()}

    def unchanged(self):
        torch.cuda.synchronize()
        return all(torch.equal(v, self.keep[k]) for k, v in self.t.items())


def ws_floats(rows, ch):
    n = int(lib().r48_bn_workspace_floats(rows, ch))
    assert n == reduce_blocks(rows, ch) * 2 * ch + 3 * ch
    return n


def forward(d, relu, with_res, with_mask, running, momentum, eps, part=None):
    """r48_bn_forward, or r48_bn_forward_stats from the records `part` [nblk, 2 C]. -> dict of save,
    coef (from the workspace), y (float64 values), ybits, mask, rm, rv (None without running)."""
    c = d.case
    rows, ch = c["rows"], c["C"]
    nws = ws_floats(rows, ch)
    ry, y = guarded(rows, torch.int16, 0x5555, row=ch)
    rk, mk = guarded(rows, torch.uint8, 0x55, row=ch // 8)
    rs, save = guarded(2 * ch, torch.float32, 7.5)
    rw, ws = guarded(nws, torch.float32, 7.5)
    rr, rm = guarded(ch, torch.float32, 7.5)
    rv_raw, rv = guarded(ch, torch.float32, 7.5)
    rm.copy_(dev(c["rm"]))
    rv.copy_(dev(c["rv"]))
    tail = (ptr(d.t["gamma"]), ptr(d.t["beta"]), ptr(rm) if running else None, ptr(rv) if running else None,
            f32(momentum), f32(eps), int(relu), ptr(save), ptr(ws), ptr(y), ptr(mk) if with_mask else None, stream())
    res = ptr(d.t["res"]) if with_res else None
    if part is None:
        check(lib().r48_bn_forward(ptr(d.t["x"]), res, rows, ch, *tail))
    else:
        tp = dev(part)
        check(lib().r48_bn_forward_stats(ptr(tp), part.shape[0], ptr(d.t["x"]), res, rows, ch, *tail))
        torch.cuda.synchronize()
        assert torch.equal(tp, dev(part))
    out = {"save": host(save).copy(), "ybits": bf16_bits(y), "y": f64(y.view(torch.bfloat16)), "mask": host(mk).copy(),
           "rm": host(rm).copy(), "rv": host(rv).copy(), "ws": host(ws).copy()}
    out["coef"] = out["ws"][nws - 3 * ch:nws - ch]
    assert guard_ok(ry, rows * ch, 0x5555) and guard_ok(rk, rows * (ch // 8) if with_mask else 0, 0x55)
    assert guard_ok(rs, 2 * ch, 7.5) and guard_ok(rw, nws, 7.5) and guard_ok(rr, ch, 7.5) and guard_ok(rv_raw, ch, 7.5)
    assert (out["ws"][nws - ch:] == 7.5).all(), "the forward writes 2 C coefficients"
    if part is not None:
        assert (out["ws"][:nws - 3 * ch] == 7.5).all(), "the record form has no statistics pass"
    if not running:
        assert (bits(out["rm"]) == bits(c["rm"])).all() and (bits(out["rv"]) == bits(c["rv"])).all()
    assert d.unchanged()
    return out


def expected_mask(y, ch):
    return np.packbits((y > 0).reshape(y.shape[0], ch // 8, 8), axis=2, bitorder="little").reshape(y.shape[0], ch // 8)


def check_forward(got, f, e, c, with_mask, running, name):
    """Every output of a forward against the reference f within the bounds e -> the worst ratio."""
    ch, x = c["C"], f64(c["x"])
    r = {"mean": worst(np.abs(got["save"][:ch] - f["mean"]), e["mean"]),
         "invstd": worst(np.abs(got["save"][ch:] - f["invstd"]), e["invstd"]),
         "a": worst(np.abs(got["coef"][:ch] - f["a"]), e["a"]), "b": worst(np.abs(got["coef"][ch:] - f["b"]), e["b"]),
         "y": y_ratio(got["y"], f, e, x)}
    if running:
        r["rm"] = worst(np.abs(got["rm"] - f["rm"]), e["rm"])
        r["rv"] = worst(np.abs(got["rv"] - f["rv"]), e["rv"])
    if with_mask:
        assert (got["mask"] == expected_mask(got["y"], ch)).all(), "%s: mask bit k of byte j != (y[8 j + k] > 0)" % name
    top = max(r, key=r.get)
    assert r[top] <= 1, "%s: %s is %.3g of its bound (%r)" % (name, top, r[top], r)
    return r


def planted_forward_facts(got, f, c, eps):
    """A constant channel: var is exactly 0, so the mean is exact and invstd = eps^-1/2 to the cast."""
    ch = c["C"]
    if c["rows"] >= 2:
        assert f["var"][CONST] == 0 and got["save"][CONST] == F32(-2.75)
        assert got["save"][ch + CONST] == F32(1.0 / np.sqrt(f32(eps)))
        assert 64 < abs(f["mean"][FAR]) / max(np.sqrt(f["var"][FAR]), 1e-30) or c["rows"] < 256


FLAGS = [(relu, res, mask) for relu in (True, False) for res in (False, True) for mask in (True, False)]


def run_forward_case(ch, rows, flags, seed):
    c = bn_case(rows, ch, seed)
    d = Device(c)
    x = f64(c["x"])
    top = {}
    for i, (relu, with_res, with_mask) in enumerate(flags):
        momentum, eps = MOM_EPS[(i + rows) % 6]
        m32, e32 = f32(momentum), f32(eps)
        f = U.bn_forward(x, f64(c["res"]) if with_res else None, c["gamma"].astype(np.float64),
                         c["beta"].astype(np.float64), c["rm"].astype(np.float64), c["rv"].astype(np.float64), m32, e32, relu)
        e = fwd_direct_bounds(f, x[0], rows, ch, c["gamma"], e32, m32)
        name = "bn forward C=%d rows=%d relu=%d res=%d mask=%d momentum=%g eps=%g" % (ch, rows, relu, with_res, with_mask,
                                                                                    momentum, eps)
        got = forward(d, relu, with_res, with_mask, True, momentum, eps)
        merge(top, check_forward(got, f, e, c, with_mask, True, name))
        planted_forward_facts(got, f, c, eps)
        if momentum == 0.0:
            assert (bits(got["rm"]) == bits(c["rm"])).all() and (bits(got["rv"]) == bits(c["rv"])).all()
        if i % 3 == 0:      # without running statistics: save, coefficients, y and mask keep their bits
            bare = forward(d, relu, with_res, with_mask, False, momentum, eps)
            for k in ("save", "coef", "ybits", "mask"):
                assert (bare[k] == got[k]).all(), "%s: %s changes without running statistics" % (name, k)
    return top


@pytest.mark.parametrize("ch,rows", SMALL)
def test_bn_forward_matches_float64_at_small_and_ragged_rows(ch, rows):
    """r48_bn_forward for relu x residual x mask-or-not (8 calls), momentum and eps cycling through
    {0.1, 0, 1} x {1e-5, 1e-3}, against update_refs.bn_forward: save {mean, invstd}, the coefficients
    (a, b) in the workspace and the running statistics within fwd_direct_bounds (the fp32 summation
    bound of the shifted sums carried through the finish), y within half a bf16 ulp + the fp32
    roundings of a x + b + res + the errors of a and b (y_ratio), every mask byte equal to the bits of
    the kernel's own y > 0. Momentum 0 leaves the running statistics' bits; without running statistics
    every other output keeps its bits. The constant channel's mean and invstd are exact. At rows = 1
    var = 0 and the running variance moves towards var itself."""
    report_all("bn forward C=%d rows=%d" % (ch, rows), run_forward_case(ch, rows, FLAGS, 1000 * ch + rows))


@pytest.mark.parametrize("ch,rows", BIG)
def test_bn_forward_matches_float64_at_the_grid_cap_and_past_it(ch, rows):
    """One combination per size (the cap: ReLU + residual + mask, the update's; past it: none of the
    three), all 1,024 reduce blocks, 4 then up to 5 rows per thread, 1,024 records for the finish's
    256 threads; bounds as at the small sizes."""
    assert reduce_blocks(rows, ch) == 1024 and chain(rows, ch) == (4 if rows % 4096 == 0 else 5)
    flags = [(True, True, True)] if rows % 4096 == 0 else [(False, False, False)]
    report_all("bn forward C=%d rows=%d" % (ch, rows), run_forward_case(ch, rows, flags, 1000 * ch + 7))


# ------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("ch", CHANNELS)
def test_bn_apply_is_bit_exact_from_hand_chosen_coefficients(ch):
    """r48_bn_apply at rows = 20 RPB + 1 for relu x residual, with the mask: a = k / 16 (|k| <= 48) and
    b fp32, so a x + b is exact in float64 and rounds once to the fused multiply-add's fp32 value; the
    residual is one fp32 add, the ReLU max(v, 0), the result rounds to nearest even bf16 -- restated in
    numpy and torch, y is bit-equal (with the ReLU up to the sign of a zero, which max leaves open).
    Channel 1: a = 1, b = -x (v = +0 exactly); channel 2: v < 0; channel 3: x = b = -0 (v = -0): their
    mask bits are 0 without a residual, and every mask byte equals the bits of y > 0."""
    rows = 20 * rpb(ch) + 1
    c = bn_case(rows, ch, 50 + ch)
    gen = torch.Generator().manual_seed(ch)
    a = (torch.randint(-48, 49, (ch,), generator=gen).float() / 16).numpy()
    b = torch.randn(ch, generator=gen).numpy()
    x = c["x"].clone()
    x[:, 2] = x[:, 2].abs()
    x[:, 3] = -0.0
    a[1], b[1], a[2], b[2], a[3], b[3] = 1.0, 2.75, -1.0, -0.5, 1.0, -0.0
    c["x"] = x
    d = Device(c)
    coef = dev(np.concatenate([a, b]).astype(F32))
    x64, r32 = f64(x), c["res"].float().numpy()
    v0 = a.astype(np.float64) * x64 + b.astype(np.float64)
    assert (v0[:, 1] == 0).all() and (v0[:, 2] < 0).all() and np.signbit(v0[:, 3]).all() and (v0[:, 3] == 0).all()
    for relu in (True, False):
        for with_res in (False, True):
            ry, y = guarded(rows, torch.int16, 0x5555, row=ch)
            rk, mk = guarded(rows, torch.uint8, 0x55, row=ch // 8)
            check(lib().r48_bn_apply(ptr(d.t["x"]), ptr(d.t["res"]) if with_res else None, rows, ch, ptr(coef), int(relu),
                                     ptr(y), ptr(mk), stream()))
            got, gotv, gm = bf16_bits(y), f64(y.view(torch.bfloat16)), host(mk)
            assert guard_ok(ry, rows * ch, 0x5555) and guard_ok(rk, rows * (ch // 8), 0x55) and d.unchanged()
            v = v0.astype(F32)
            if with_res:
                v = v + r32
            if relu:
                v = np.where(v > 0, v, F32(0))
            want = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            if relu:
                got = np.where(got == 0x8000, 0, got)
            assert (got == want).all(), "bn apply C=%d relu=%d res=%d: %d entries differ" % (ch, relu, with_res,
                                                                                           (got != want).sum())
            assert (gm == expected_mask(gotv, ch)).all()
            if not with_res:
                assert (mask_bits(gm, ch)[:, 1:4] == 0).all(), "a zero or a negative value sets no mask bit"
                assert (got[:, 3] == (0 if relu else 0x8000)).all()
    report("bn apply C=%d (bit-exact)" % ch, 0.0)


# ------------------------------------------------------------------------------------ backward
def grad_through(c, form):
    """(g, passed): the gradient the backward sums -- dy where y > 0 ('y'), where the mask bit is set
    ('mask'), or dy itself ('none'), 0 elsewhere -- and where it passes. Exact."""
    dy = f64(c["dy"])
    if form == "y":
        passed = f64(c["y"]) > 0
    elif form == "mask":
        passed = mask_bits(c["mask"].numpy(), c["C"])
    else:
        passed = np.ones(dy.shape, bool)
    return np.where(passed, dy, 0.0), passed


def backward(d, form, with_dres, save, part=None):
    """r48_bn_backward (form 'y', 'mask' or 'none'), or r48_bn_backward_part from the records `part`. ->
    dict of dx (float64), dxbits, dres bits, dgamma, dbeta, coef (from the workspace), ws."""
    c = d.case
    rows, ch = c["rows"], c["C"]
    nws = ws_floats(rows, ch)
    rx, dx = guarded(rows, torch.int16, 0x5555, row=ch)
    rd, dres = guarded(rows, torch.int16, 0x5555, row=ch)
    rg, dgb = guarded(2 * ch, torch.float32, 7.5)
    rw, ws = guarded(nws, torch.float32, 7.5)
    ts = dev(save)
    tail = (ptr(dx), ptr(dres) if with_dres else None, ptr(dgb), ptr(dgb[ch:]), stream())
    if part is None:
        check(lib().r48_bn_backward(ptr(d.t["dy"]), ptr(d.t["y"]) if form == "y" else None,
                                    ptr(d.t["mask"]) if form == "mask" else None, ptr(d.t["x"]), rows, ch, ptr(d.t["gamma"]),
                                    ptr(ts), int(form != "none"), ptr(ws), *tail))
    else:
        tp = dev(part)
        check(lib().r48_bn_backward_part(ptr(tp), part.shape[0], ptr(d.t["dy"]), ptr(d.t["mask"]), ptr(d.t["x"]), rows, ch,
                                         ptr(d.t["gamma"]), ptr(ts), ptr(ws), *tail))
        torch.cuda.synchronize()
        assert torch.equal(tp, dev(part))
    out = {"dxbits": bf16_bits(dx), "dx": f64(dx.view(torch.bfloat16)), "dres": bf16_bits(dres), "dgamma": host(dgb)[:ch].copy(),
           "dbeta": host(dgb)[ch:].copy(), "ws": host(ws).copy()}
    out["coef"] = out["ws"][nws - 3 * ch:]
    assert guard_ok(rx, rows * ch, 0x5555) and guard_ok(rd, rows * ch if with_dres else 0, 0x5555)
    assert guard_ok(rg, 2 * ch, 7.5) and guard_ok(rw, nws, 7.5)
    if part is not None:
        assert (out["ws"][:nws - 3 * ch] == 7.5).all(), "the record form has no reduction pass"
    assert d.unchanged() and torch.equal(ts, dev(save))
    return out


def check_backward(got, b, e, c, g, passed, with_dres, name, want_dx=None):
    ch, x = c["C"], f64(c["x"])
    want_dx = b["dx"] if want_dx is None else want_dx
    r = {"dbeta": worst(np.abs(got["dbeta"] - b["dbeta"]), e["dbeta"]),
         "dgamma": worst(np.abs(got["dgamma"] - b["dgamma"]), e["dgamma"]),
         "a": worst(np.abs(got["coef"][:ch] - b["a"]), e["a"]), "cc": worst(np.abs(got["coef"][ch:2 * ch] - b["cc"]), e["cc"]),
         "d": worst(np.abs(got["coef"][2 * ch:] - b["d"]), e["d"]), "dx": dx_ratio(got["dx"], want_dx, b, e, g, x)}
    if with_dres:       # bf16(g): the bits of dy where the ReLU passes it (a zero keeps its sign), +0 elsewhere
        dyb = c["dy"].view(torch.int16).numpy().view(np.uint16)
        assert (got["dres"] == np.where(passed, dyb, 0)).all(), "%s: dresidual != bf16(g)" % name
    top = max(r, key=r.get)
    assert r[top] <= 1, "%s: %s is %.3g of its bound (%r)" % (name, top, r[top], r)
    return r


def saved_stats(c):
    """The float64 mean and invstd of the case's x (eps 1e-5) and their fp32 save."""
    x = f64(c["x"])
    mean = x.mean(0)
    invstd = 1.0 / np.sqrt(np.square(x - mean).mean(0) + f32(1e-5))
    return mean, invstd, np.concatenate([mean, invstd]).astype(F32)


def run_backward_case(ch, rows, combos, seed):
    c = bn_case(rows, ch, seed)
    d = Device(c)
    x = f64(c["x"])
    mean, invstd, save = saved_stats(c)
    top = {}
    for form, with_dres in combos:
        g, passed = grad_through(c, form)
        b = U.bn_backward(g, x, mean, invstd, c["gamma"].astype(np.float64))
        e = bwd_direct_bounds(b, rows, ch, mean, invstd)
        name = "bn backward C=%d rows=%d form=%s dres=%d" % (ch, rows, form, with_dres)
        got = backward(d, form, with_dres, save)
        merge(top, check_backward(got, b, e, c, g, passed, with_dres, name))
        if rows >= 2:
            assert got["dgamma"][CONST] == 0, "a constant channel has x - mean = 0 exactly"
        if form != "none":
            k = ch - 1
            assert (g[:, k] == 0).all() and got["dbeta"][k] == 0 and got["dgamma"][k] == 0 and (got["dx"][:, k] == 0).all()
        assert (got["dx"][:, G0] == 0).all()
    return top


BWD_COMBOS = [(form, dres) for form in ("y", "mask", "none") for dres in (False, True)]


@pytest.mark.parametrize("ch,rows", SMALL)
def test_bn_backward_matches_float64_at_small_and_ragged_rows(ch, rows):
    """r48_bn_backward with the ReLU from y, from random mask bytes (y = NULL) and without, each with
    and without dresidual, against update_refs.bn_backward of the exactly masked gradient, the float64
    statistics of x as its mean and invstd and their fp32 roundings as the kernel's save: dbeta, dgamma
    and the coefficients (a, cc, d) in the workspace within bwd_direct_bounds (the fp32 summation bound,
    the u |mean| sum |g| of the fp32 mean, carried through the finish), dx within half a bf16 ulp + the
    fp32 roundings of a g + cc x + d + the coefficients' errors (dx_ratio), dresidual bit-equal to
    bf16(g). The constant channel's dgamma is exactly 0; the channel whose mask bits are all 0 (whose
    y is <= 0) has dbeta = dgamma = 0 and dx = 0; gamma = 0 gives dx = 0."""
    report_all("bn backward C=%d rows=%d" % (ch, rows), run_backward_case(ch, rows, BWD_COMBOS, 2000 * ch + rows))


@pytest.mark.parametrize("ch,rows", BIG)
def test_bn_backward_matches_float64_at_the_grid_cap_and_past_it(ch, rows):
    """One combination per size (the cap: the mask form with dresidual, the update's; past it: the
    ReLU from y, no dresidual); bounds as at the small sizes."""
    combos = [("mask", True)] if rows % 4096 == 0 else [("y", False)]
    report_all("bn backward C=%d rows=%d" % (ch, rows), run_backward_case(ch, rows, combos, 2000 * ch + 7))


# ----------------------------------------------------------------------------- the record forms
NBLK = [1, 255, 256, 257, 1024]
T64 = 16 * D53      # 1,024 records in float64: 4 per thread in a chain, 8 tree levels, and numpy's own sum


def records(cols, rows, nblk):
    """cols [rows, K] float64 -> fp32 [nblk, K]: the sums of nblk consecutive chunks of rows (chunk k
    is rows k rows / nblk .. (k + 1) rows / nblk: empty ones give 0; the last one ends with the last row)."""
    cs = np.concatenate([np.zeros((1, cols.shape[1])), np.cumsum(cols, 0)])
    edge = (np.arange(nblk + 1) * rows) // nblk
    return (cs[edge[1:]] - cs[edge[:-1]]).astype(F32)


@pytest.mark.parametrize("nblk", NBLK)
@pytest.mark.parametrize("ch", CHANNELS)
def test_bn_record_forms_match_float64_of_the_same_records(ch, nblk):
    """r48_bn_finish, r48_bn_forward_stats, r48_bn_backward_part and r48_bn_backward_apply from records
    the test makes: the rows (1 and 20 RPB + 1) split into nblk chunks, each chunk's float64 sums (x and
    x^2 forward; g and g (x - mean) backward, g through random mask bytes, mean the fp32 save) rounded to
    fp32. The reference is update_refs.bn_from_sums / bn_backward_from_sums of the float64 sum of those
    same fp32 records, so each output is within one fp32 rounding, plus 16 2^-53 sum |record| for the
    order of the float64 sum and 4 2^-53 (S2 / n + mean^2) for the cancellation of S2 / n - mean^2,
    carried through as in fwd_bounds / bwd_bounds. y and dx as in the direct tests; r48_bn_finish's
    save, coefficients and running statistics are bit-equal to r48_bn_forward_stats'; r48_bn_backward_apply
    from r48_bn_backward_part's coefficients gives its dx bit for bit. The channel that is zero but for
    its last row has its whole mass in the last record: at nblk = 257 that is record 256, the first one
    of the finish threads' second trip."""
    top = {}
    for rows in (1, 20 * rpb(ch) + 1):
        c = bn_case(rows, ch, 3000 * ch + nblk + rows)
        d = Device(c)
        x = f64(c["x"])
        momentum, eps = MOM_EPS[(nblk + rows) % 6]
        m32, e32 = f32(momentum), f32(eps)
        part = records(np.concatenate([x, x * x], 1), rows, nblk)
        assert part.shape == (nblk, 2 * ch) and (part[:-1, LAST] == 0).all() and part[-1, LAST] != 0
        s = part.astype(np.float64).sum(0)
        mag = np.abs(part.astype(np.float64)).sum(0)
        f = U.bn_from_sums(s[:ch], s[ch:], rows, 0.0, c["gamma"].astype(np.float64), c["beta"].astype(np.float64),
                           c["rm"].astype(np.float64), c["rv"].astype(np.float64), m32, e32)
        e_dm = T64 * mag[:ch] / rows
        e_var = T64 * mag[ch:] / rows + 2 * np.abs(f["mean"]) * e_dm + 4 * D53 * (s[ch:] / rows + f["mean"] ** 2)
        e = fwd_bounds(f, rows, e_dm, e_var, c["gamma"], e32, m32)
        relu, with_res = nblk % 2 == 1, nblk != 256
        f["z"] = f["a"] * x + f["b"] + (f64(c["res"]) if with_res else 0.0)
        f["z_mag"] = np.abs(f["a"] * x) + np.abs(f["b"]) + (np.abs(f64(c["res"])) if with_res else 0.0)
        f["y"] = np.maximum(f["z"], 0.0) if relu else f["z"]
        name = "bn records C=%d nblk=%d rows=%d" % (ch, nblk, rows)
        got = forward(d, relu, with_res, True, True, momentum, eps, part=part)
        merge(top, check_forward(got, f, e, c, True, True, name + " forward_stats"))
        # r48_bn_finish alone
        tp = dev(part)
        rs, save = guarded(2 * ch, torch.float32, 7.5)
        rc, coef = guarded(2 * ch, torch.float32, 7.5)
        rr, run = guarded(2 * ch, torch.float32, 7.5)
        run.copy_(dev(np.concatenate([c["rm"], c["rv"]])))
        check(lib().r48_bn_finish(ptr(tp), nblk, rows, ch, ptr(d.t["gamma"]), ptr(d.t["beta"]), ptr(run), ptr(run[ch:]),
                                  m32, e32, ptr(save), ptr(coef), stream()))
        assert guard_ok(rs, 2 * ch, 7.5) and guard_ok(rc, 2 * ch, 7.5) and guard_ok(rr, 2 * ch, 7.5)
        assert torch.equal(tp, dev(part)) and d.unchanged()
        assert (bits(host(save)) == bits(got["save"])).all() and (bits(host(coef)) == bits(got["coef"])).all()
        assert (bits(host(run)) == bits(np.concatenate([got["rm"], got["rv"]]))).all()
        # backward: records of g and g (x - mean) with the fp32 save as the mean
        _, _, save32 = saved_stats(c)
        mean, invstd = save32[:ch].astype(np.float64), save32[ch:].astype(np.float64)
        g, passed = grad_through(c, "mask")
        bpart = records(np.concatenate([g, g * (x - mean)], 1), rows, nblk)
        sb, magb = bpart.astype(np.float64).sum(0), np.abs(bpart.astype(np.float64)).sum(0)
        b = U.bn_backward_from_sums(sb[:ch], sb[ch:], rows, mean, invstd, c["gamma"].astype(np.float64))
        eb = bwd_bounds(b, rows, ch, mean, invstd, T64 * magb[:ch], T64 * magb[ch:], True)
        with_dres = nblk % 2 == 0
        gotb = backward(d, "mask", with_dres, save32, part=bpart)
        want_dx = b["a"] * g + b["cc"] * x + b["d"]
        merge(top, check_backward(gotb, b, eb, c, g, passed, with_dres, name + " backward_part", want_dx=want_dx), "bwd ")
        rx, dx = guarded(rows, torch.int16, 0x5555, row=ch)
        tc = dev(gotb["coef"])
        check(lib().r48_bn_backward_apply(ptr(d.t["dy"]), ptr(d.t["mask"]), ptr(d.t["x"]), rows, ch, ptr(tc), ptr(dx),
                                          stream()))
        assert (bf16_bits(dx) == gotb["dxbits"]).all() and guard_ok(rx, rows * ch, 0x5555) and d.unchanged()
    report_all("bn records C=%d nblk=%d" % (ch, nblk), top)


# ------------------------------------------------------------------------------ argument checks
def test_bn_entries_refuse_bad_arguments_and_write_nothing():
    """R48_EINVAL without a launch: C = 48, rows = 0, a pointer 2 bytes off (x, y, the residual, dy, dx),
    running_mean without running_var and the other way round, a ReLU backward with neither y nor mask,
    nblk = 0 in the three record forms. Every output buffer keeps its poison."""
    from rein48_amd import _lib
    rows, ch = 8, 64
    c = bn_case(rows + 1, ch, 9)
    d = Device(c)
    t, L, s, bad = d.t, lib(), stream(), _lib.R48_EINVAL
    outs = [torch.full((rows + 1, ch), 0x5555, dtype=torch.int16, device=DEV) for _ in range(3)]
    fl = [torch.full((8 * ch,), 7.5, dtype=torch.float32, device=DEV) for _ in range(5)]
    mk = torch.full((rows + 1, ch // 8), 0x55, dtype=torch.uint8, device=DEV)
    y, dx, dres = outs
    save, ws, run, coef, grads = fl
    part = torch.zeros(4, 2 * ch, device=DEV)

    def off(tensor):
        return C.c_void_p(tensor.data_ptr() + 2)

    def fwd(x=None, res=None, n=rows, cc=ch, rm=None, rv=None, yy=None):
        return L.r48_bn_forward(x or ptr(t["x"]), res, n, cc, ptr(t["gamma"]), ptr(t["beta"]), rm, rv, 0.1, 1e-5, 1,
                                ptr(save), ptr(ws), yy or ptr(y), ptr(mk), s)

    def fwd_stats(nblk=4, n=rows, cc=ch, x=None):
        return L.r48_bn_forward_stats(ptr(part), nblk, x or ptr(t["x"]), None, n, cc, ptr(t["gamma"]), ptr(t["beta"]), None,
                                      None, 0.1, 1e-5, 1, ptr(save), ptr(ws), ptr(y), ptr(mk), s)

    def finish(nblk=4, n=rows, cc=ch, rm=None, rv=None):
        return L.r48_bn_finish(ptr(part), nblk, n, cc, ptr(t["gamma"]), ptr(t["beta"]), rm, rv, 0.1, 1e-5, ptr(save),
                               ptr(coef), s)

    def bwd(dy=None, yy="y", mask=None, n=rows, cc=ch, relu=1, out=None, dr=None):
        return L.r48_bn_backward(dy or ptr(t["dy"]), ptr(t["y"]) if yy == "y" else yy, mask, ptr(t["x"]), n, cc,
                                 ptr(t["gamma"]), ptr(save), relu, ptr(ws), out or ptr(dx), dr, ptr(grads), ptr(grads[ch:]), s)

    def bwd_part(nblk=4, n=rows, cc=ch, out=None):
        return L.r48_bn_backward_part(ptr(part), nblk, ptr(t["dy"]), ptr(t["mask"]), ptr(t["x"]), n, cc, ptr(t["gamma"]),
                                      ptr(save), ptr(ws), out or ptr(dx), None, ptr(grads), ptr(grads[ch:]), s)

    def apply(n=rows, cc=ch, x=None, yy=None):
        return L.r48_bn_apply(x or ptr(t["x"]), None, n, cc, ptr(coef), 1, yy or ptr(y), ptr(mk), s)

    def bwd_apply(n=rows, cc=ch, out=None, dy=None):
        return L.r48_bn_backward_apply(dy or ptr(t["dy"]), ptr(t["mask"]), ptr(t["x"]), n, cc, ptr(coef), out or ptr(dx), s)
    calls = {
        "C = 48": [fwd(cc=48), fwd_stats(cc=48), finish(cc=48), bwd(cc=48), bwd_part(cc=48), apply(cc=48), bwd_apply(cc=48)],
        "rows = 0": [fwd(n=0), fwd_stats(n=0), finish(n=0), bwd(n=0), bwd_part(n=0), apply(n=0), bwd_apply(n=0)],
        "2 bytes off": [fwd(x=off(t["x"])), fwd(res=off(t["res"])), fwd(yy=off(y)), fwd_stats(x=off(t["x"])),
                        bwd(dy=off(t["dy"])), bwd(out=off(dx)), bwd(dr=off(dres)), bwd(yy=off(t["y"])),
                        bwd_part(out=off(dx)), apply(x=off(t["x"])), apply(yy=off(y)), bwd_apply(out=off(dx)),
                        bwd_apply(dy=off(t["dy"]))],
        "one running statistic": [fwd(rm=ptr(run)), fwd(rv=ptr(run)), finish(rm=ptr(run)), finish(rv=ptr(run))],
        "relu without y or mask": [bwd(yy=None)],
        "nblk = 0": [fwd_stats(nblk=0), finish(nblk=0), bwd_part(nblk=0)],
    }
    for what, codes in calls.items():
        assert all(code == bad for code in codes), "%s: %r" % (what, codes)
    assert L.r48_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 0x5555).all()) for o in outs) and all(bool((v == 7.5).all()) for v in fl)
    assert bool((mk == 0x55).all()) and d.unchanged()
    check(bwd(yy=None, relu=0))       # and the same call without the ReLU is accepted
    torch.cuda.synchronize()
    assert not bool((dx[:rows] == 0x5555).all()) and bool((dx[rows:] == 0x5555).all())
