"""The 3x3 conv kernels of rein48_amd/csrc/r48_conv.hip -- k_conv3x3 in its eight instantiations, k_conv_wgrad
and k_conv_wgrad_reduce -- each C-ABI entry against the float64 references of tests/update_refs.py (conv3x3,
conv3x3_dgrad, conv3x3_wgrad, held to torch's conv2d + autograd by test_update_kernels_host.py and evaluated
here with torch float64 on the device), entry by entry, at the smallest board counts that reach every tile,
tail and ring position.

Conventions (test_update_kernels_gpu.py's and test_bn_kernels_gpu.py's): every output is a slice of a
poisoned buffer whose guard is checked, inputs are compared with their originals after the call, every
entry is checked, and each test prints its worst error / bound ratio. u = 2^-24 is fp32's unit roundoff; a
bound is a count K of fp32 roundings times the sum of the magnitudes of the terms (`mag`), stated in the
docstrings. Nothing here is a tolerance measured on the device.

Two kinds of input.
  exact  x, dy, add, bn_x in {-4..4} / 4, w in {-8..8} / 8, bias in {-32..32} / 4, means k / 4: every product
         and partial sum is a multiple of 2^-5 (2^-4 in the weight gradient) and the sums of magnitudes stay
         below 2^24 of that unit (asserted on the inputs before the launch), so fp32 accumulation is exact in
         any order and at any internal width of the MFMA: bf16 outputs must equal the float64 result rounded
         once (a zero's sign left open), dw the float64 result itself. Any indexing fault is a bit mismatch.
  real   N(0, 1) activations with +-0 sprinkled in, w ~ 0.1 N(0, 1) rounded to bf16, bias around +-2, every
         magnitude in [2^-8, 2^6] or 0 (no subnormal enters an MFMA): |got - want| <= out_bound(want, K u mag)
         per entry for bf16 outputs, K u mag + u |want| for fp32 ones.

K of each bound, from the kernel:
  conv (forward, data gradient)   9 cin + 2: an accumulator starts at the bias (or +0) and takes the cin
      products of each of at most 9 in-grid taps through the MFMAs (the products of two bf16 are exact in
      fp32; each is counted as one rounding of the running sum, whatever the MFMA's internal order), then
      the add: 9 cin + 1 additions, one more for the start.
  statistics records              32 T + 3 + 8: a lane adds one value per channel for each of the 8 pieces of
      each of the 4 rows of each of its T = ceil(tiles / 2048) tiles (the square enters fused), then 3
      shuffle levels (lanes l ^ 8, 16, 32) and the 8 waves in order. One more in sum g (x - mean) for the
      fp32 x - mean. The records are summed in float64 (by the test, and by the finishing workgroup).
  weight gradient                 32 kPer n + (kSplit - 1) + 32: an accumulator takes kPer MFMAs of 32 rows in
      each of the workgroup's n = ceil(steps / 256) steps, the kSplit waves of a channel tile are added
      through LDS, and records_sum16 adds 16 records then 16 groups (kSplit = 128 / cin, kPer = 4 / kSplit).
  the finishing forms             fwd_bounds / bwd_bounds of test_bn_kernels_gpu.py over the float64 sum of the
      kernel's own fp32 records, whose order (64 records per thread in a chain, 3 adds of the quarters, the
      test's own sum) is worth TFIN = 80 2^-53 of the summed magnitudes.

Geometry. k_conv3x3: a tile is 16 boards, a wave takes tile 8 blockIdx + wave then + 8 gridDim; the plain form
launches ceil(tiles / 8) <= 256 workgroups, the forms with statistics always 256. Board counts 1, 2, 15, 16,
17, 33, 128, 129 (the plain form's second workgroup) and 32,785 = 2,048 x 16 + 17 (wave 0's second tile is
full, wave 1's has one live board: the cross-tile prefetch and the tile loop), exact inputs at every size,
real ones at 1, 17, 129 and 32,785. k_conv_wgrad: a step is 8 boards, workgroup b takes steps b, b + 256,
...; the ring has 3 buffers. Board counts 1, 7, 8, 9, 2,047, 2,048, 2,049, 4,097, 6,144, 6,145 (workgroup 0's
fourth step, ragged, in a ring buffer already used once) and 6,160; real inputs at 1, 9, 2,049, 6,145, 6,160.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import update_refs as U
from test_bn_kernels_gpu import D53, MOM_EPS, SLACK, bwd_bounds, f32, fwd_bounds, merge, out_bound, report_all
from test_ntuple_gpu import guard_ok, guarded
from test_update_kernels_gpu import DEV, check, host, lib, ptr, stream, worst

pytestmark = pytest.mark.gpu
u = U.U
F32 = np.float32
BF = torch.bfloat16
NREC = 256                      # workgroups of the persistent forms = statistics / weight-gradient records
TFIN = 80 * D53                 # the float64 sums over the records (module docstring)
ALL0, ALL1, LASTBIT = 5, 14, 23  # planted mask columns: every bit 0, every bit 1, only the last row's bit
CONV_BOARDS = [1, 2, 15, 16, 17, 33, 128, 129, 32785]
CONV_REAL = [1, 17, 129, 32785]
WGRAD_BOARDS = [1, 7, 8, 9, 2047, 2048, 2049, 4097, 6144, 6145, 6160]
WGRAD_REAL = [1, 9, 2049, 6145, 6160]
FIN_BOARDS = [1, 17, 129]


def kinds(B, real_at):
    return ["exact"] + (["real"] if B in real_at else [])


# ------------------------------------------------------------------------------------ the inputs
def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def in_range(t):
    """Magnitudes moved into [2^-8, 2^6], signs kept."""
    return torch.copysign(t.abs().clamp(2.0 ** -8, 2.0 ** 6), t)


def act(kind, shape, g):
    """bf16 activations on the device: {-4..4} / 4, or N(0, 1) within [2^-8, 2^6] with 5 % +0 and 5 % -0."""
    if kind == "exact":
        return (torch.randint(-4, 5, shape, generator=g, device=DEV).float() / 4).to(BF)
    t = in_range(torch.randn(shape, generator=g, device=DEV))
    z = torch.rand(shape, generator=g, device=DEV)
    t[z < 0.05] = 0.0
    t[z > 0.95] = -0.0
    return t.to(BF)


@functools.lru_cache(None)
def weights(kind, cin):
    """(w fp32 [64, cin, 3, 3] of bf16 values, bias fp32 [64]) on the device; the same for every test."""
    g = gen(100 * cin + (kind == "real"))
    if kind == "exact":
        w = torch.randint(-8, 9, (64, cin, 3, 3), generator=g, device=DEV).float() / 8
        bias = torch.randint(-32, 33, (64,), generator=g, device=DEV).float() / 4
    else:
        w = in_range(0.1 * torch.randn((64, cin, 3, 3), generator=g, device=DEV)).to(BF).float()
        sign = torch.where(torch.rand(64, generator=g, device=DEV) < 0.5, -1.0, 1.0)
        bias = in_range(torch.randn(64, generator=g, device=DEV) * 0.5 + 2.0) * sign
    return w.contiguous(), bias.contiguous()


@functools.lru_cache(None)
def frags(kind, cin, dgrad=False):
    from rein48_amd.dqn.conv import pack_conv, pack_conv_dgrad
    w = weights(kind, cin)[0]
    return pack_conv_dgrad(w) if dgrad else pack_conv(w, cin)


def random_mask(rows, g):
    """uint8 [rows, 8] (bit k of byte j = channel 8 j + k) with the planted columns ALL0, ALL1, LASTBIT."""
    m = torch.randint(0, 256, (rows, 8), generator=g, device=DEV, dtype=torch.uint8)
    m[:, ALL0 // 8] &= 0xFF ^ (1 << ALL0 % 8)
    m[:, ALL1 // 8] |= 1 << ALL1 % 8
    m[:, LASTBIT // 8] &= 0xFF ^ (1 << LASTBIT % 8)
    m[rows - 1, LASTBIT // 8] |= 1 << LASTBIT % 8
    return m


def mask_bool(m):
    """uint8 [rows, 8] -> bool [rows, 64]."""
    return ((m.long().unsqueeze(-1) >> torch.arange(8, device=DEV)) & 1).bool().reshape(m.shape[0], 64)


def mask_of(zbits):
    """int16 bf16 bits [rows, 64] -> the mask bytes [rows, 8] of z > 0."""
    pos = (zbits.view(BF) > 0).view(-1, 8, 8).to(torch.int32)
    return (pos << torch.arange(8, device=DEV, dtype=torch.int32)).sum(2).to(torch.uint8)


class Kept:
    """Input tensors with the copies that show they were left alone."""

    def __init__(self, **t):
        self.t = {k: v for k, v in t.items() if v is not None}
        self.keep = {k: v.clone() for k, v in self.t.items()}

    def unchanged(self):
        torch.cuda.synchronize()
        return all(torch.equal(v.view(torch.uint8), self.keep[k].view(torch.uint8)) for k, v in self.t.items())


# ------------------------------------------------------------------------------------ the checks
def multiple_of(t, unit):
    v = t.double() / unit
    return bool((v == v.round()).all())


def assert_exact(mag, unit, what):
    """The precondition of a bit-exact fp32 sum: sum |terms| / unit < 2^24 (the terms multiples of unit)."""
    assert float(mag.max()) / unit < 2.0 ** 24, "%s: the exact inputs do not keep fp32 exact" % what


def i16(t):
    return t.reshape(-1).view(torch.int16)


def same_bits(got, want, name):
    """got (bf16 bits, int16) == want (float64, exact in fp32) rounded once to bf16, a zero's sign left open."""
    g, w = i16(got), i16(want.float().to(BF))
    g, w = torch.where(g == -32768, 0, g), torch.where(w == -32768, 0, w)
    n = int((g != w).sum())
    assert n == 0, "%s: %d of %d entries differ from the float64 result rounded once to bf16" % (name, n, g.numel())
    return 0.0


def half_ulp(v):
    """update_refs.bf16_half_ulp on the device (v >= 0, float64): 2^(e - 9) built from its exponent bits."""
    _, e = torch.frexp(v)
    return torch.where(v > 0, ((e.long() + (1023 - 9)) << 52).view(torch.float64), torch.zeros_like(v))


def bf16_ratio(got, want, e32):
    """max |got - want| / out_bound(want, e32) over every entry (test_update_kernels_gpu.worst's rules),
    evaluated on the device; the bound's first entries are held to test_bn_kernels_gpu.out_bound itself."""
    got, want, e32 = got.reshape(-1), want.reshape(-1), e32.reshape(-1)
    bound = half_ulp(want.abs() + e32) + e32
    k = min(4096, bound.numel())
    assert (host(bound[:k]) == out_bound(host(want[:k]), host(e32[:k]))).all()
    err = (got - want).abs()
    assert not bool(torch.isnan(err).any())
    r = torch.where(err == 0, 0.0, err / torch.where(bound > 0, bound, 1.0))
    r = torch.where((err > 0) & (bound <= 0), float("inf"), r)
    return float(r.max())


def check_bf16(kind, got, want, mag, K, unit, name):
    """A bf16 output [.., 64] (int16 bits) against the float64 want: bit-equal (exact inputs, unit the
    terms' common divisor) or within out_bound(want, K u mag) (real inputs) -> the worst ratio."""
    if kind == "real":
        r = bf16_ratio(got.view(BF).double(), want, K * u * SLACK * mag)
        assert r <= 1, "%s: %.3g of the bound" % (name, r)
        return r
    assert multiple_of(want, unit)
    assert_exact(mag, unit, name)
    return same_bits(got, want, name)


def tiles_per_wave(B):
    return -(-(-(-B // 16)) // (8 * NREC))


def new_stats():
    """A guarded statistics buffer poisoned with NaN, its last 4 floats (the arrival counter and its pad) 0."""
    n = int(lib().r48_conv_stats_floats())
    assert n == NREC * 128 + 4
    raw, st = guarded(n, torch.float32, 7.5)
    st.fill_(float("nan"))
    st[NREC * 128:] = 0.0
    return raw, st


def stats_records(raw, st, B):
    """The 256 records [256, 2, 64] of a statistics buffer after a launch: all finite, those of workgroups
    without a tile exactly 0, the arrival counter and its 3 pad floats 0 bits, the guard whole."""
    n = NREC * 128 + 4
    assert guard_ok(raw, n, 7.5)
    h = host(st)
    rec = h[:NREC * 128].reshape(NREC, 2, 64)
    assert np.isfinite(rec).all(), "a workgroup left its record unwritten"
    busy = -(-(-(-B // 16)) // 8)
    assert (rec[busy:] == 0).all(), "a workgroup without a tile writes a zero record"
    assert (h[NREC * 128:].view(np.int32) == 0).all(), "the arrival counter and its pad"
    return rec


def records_ratio(rec, t1, t2, K1, K2, units, name):
    """The float64 sum of the records against the float64 sums of the terms t1, t2 [rows, 64] (device,
    float64): within K u sum |terms| (+ 2 (rows + 256) 2^-53 of it for the two float64 sums), and exactly
    equal where the terms are multiples of units = (unit1, unit2) and sum |terms| / unit < 2^24. A channel
    with at most one non-zero term has nothing to round: its first sum is exact."""
    rows = t1.shape[0]
    got = rec.astype(np.float64).sum(0)
    out = {}
    for i, (t, K) in enumerate(((t1, K1), (t2, K2))):
        want, mag = host(t.sum(0)), host(t.abs().sum(0))
        err = np.abs(got[i] - want)
        out["s%d" % (i + 1)] = worst(err, (K * u * SLACK + 2 * (rows + NREC) * D53) * mag)
        if units is not None and multiple_of(t, units[i]):
            provable = mag / units[i] < 2.0 ** 24
            assert (err[provable] == 0).all(), "%s: sum %d is not exact where fp32 must be" % (name, i + 1)
            out["exact s%d" % (i + 1)] = 0.0
        if i == 0:
            single = host((t != 0).sum(0)) <= 1
            assert (err[single] == 0).all(), "%s: a sum of one term is that term" % name
    top = max(out, key=out.get)
    assert out[top] <= 1, "%s: %s is %.3g of its bound" % (name, top, out[top])
    return out


def y_stats_ratio(rec, ybits, B, unit, name):
    """The records of SM = 1 against the sums of the kernel's own bf16 y and y^2."""
    y = ybits.view(BF).double().reshape(-1, 64)
    K = 32 * tiles_per_wave(B) + 3 + 8
    return records_ratio(rec, y, y * y, K, K, None if unit is None else (unit, unit * unit), name)


# ------------------------------------------------------------------------------------ the calls
def conv(x, B, cin, fr, bias, add, stats):
    """r48_conv3x3 into a guarded y -> its bf16 bits (int16 [B, 1024])."""
    raw, y = guarded(B, torch.int16, 0x5555, row=1024)
    check(lib().r48_conv3x3(ptr(x), B, cin, ptr(fr), ptr(bias), ptr(add), ptr(y), ptr(stats), stream()))
    torch.cuda.synchronize()
    assert guard_ok(raw, B * 1024, 0x5555), "r48_conv3x3 wrote past y"
    return y


def fin_args(gamma, beta, rm, rv, save, coef, dgamma, dbeta, rows, momentum, eps):
    from rein48_amd import _lib

    def p(t):
        return None if t is None else t.data_ptr()
    return _lib.BnFinishArgs(p(gamma), p(beta), p(rm), p(rv), p(save), p(coef), p(dgamma), p(dbeta), rows, momentum, eps)


# ------------------------------------------------------------------------------- weight fragments
def test_conv_pack_resnet_gives_the_fragments_these_tests_use():
    """r48_conv_pack_resnet (the update's packing launch) on the weights of this file -- the 64-channel
    exact and real ones as conv1 and conv2, the first 18 input channels of the 32-channel ones as the stem
    -- gives the bits of pack_conv / pack_conv_dgrad, which every other test here feeds the kernels."""
    from rein48_amd.dqn.conv import pack_conv, pack_resnet_train
    ws = [weights("exact", 32)[0][:, :18].contiguous(), weights("exact", 64)[0], weights("real", 64)[0]]
    ws += [weights("real", 64)[0].flip(0).contiguous() for _ in range(6)]
    keep = [w.clone() for w in ws]
    fwd, dg = pack_resnet_train([types.SimpleNamespace(weight=w) for w in ws])
    torch.cuda.synchronize()
    assert torch.equal(fwd[0].view(-1), pack_conv(ws[0], 32).view(-1))
    for i, kind in ((1, "exact"), (2, "real")):
        assert torch.equal(fwd[i].view(-1), frags(kind, 64).view(-1)), kind
        assert torch.equal(dg[i].view(-1), frags(kind, 64, True).view(-1)), kind
    stem_real = pack_conv(weights("real", 32)[0][:, :18].contiguous(), 32).view(36, 64, 8)
    full_real = frags("real", 32).view(36, 64, 8)
    g8 = 8 * (torch.arange(64, device=DEV) >> 4)[:, None] + torch.arange(8, device=DEV)[None, :]     # input channel
    assert torch.equal(torch.where(g8 < 18, full_real, 0), stem_real), "a fragment's element (l, j) is channel 8 (l >> 4) + j"
    assert all(torch.equal(a, b) for a, b in zip(ws, keep))


# ------------------------------------------------------------------------------------- 1. forward
def forward_case(kind, B, cin, top):
    w, bias = weights("real" if kind == "real" else "exact", cin)
    fr = frags("real" if kind == "real" else "exact", cin)
    g = gen(7 * B + cin + (kind == "real"))
    if kind == "onehot":
        boards = torch.randint(0, 18, (B, 16), generator=g, device=DEV).to(torch.int8)
        raw, xo = guarded(B, torch.int16, 0x5555, row=512)
        check(lib().r48_board_onehot32(ptr(boards), B, ptr(xo), stream()))
        assert guard_ok(raw, B * 512, 0x5555)
        x = xo.view(BF).view(B, 16, 32)
        assert bool((x.float().sum(2) == 1).all()) and bool((x[:, :, 18:] == 0).all())
    else:
        x = act(kind, (B, 16, cin), g)
    k = Kept(x=x, w=fr, bias=bias)
    for with_bias in (True, False):
        b = bias if with_bias else None
        name = "conv forward %s B=%d cin=%d bias=%d" % (kind, B, cin, with_bias)
        want, mag = U.conv3x3(x.double(), w.double(), None if b is None else b.double())
        y = conv(x, B, cin, fr, b, None, None)
        r = check_bf16(kind, y, want, mag, 9 * cin + 2, 2.0 ** -5, name)
        raw, st = new_stats()
        ys = conv(x, B, cin, fr, b, None, st)
        assert torch.equal(y, ys), "%s: the output changes with stats" % name
        rec = stats_records(raw, st, B)
        merge(top, {"y": r})
        merge(top, y_stats_ratio(rec, ys, B, None if kind == "real" else 2.0 ** -5, name), "stats ")
        del want, mag
    assert k.unchanged()


@pytest.mark.parametrize("B", CONV_BOARDS)
@pytest.mark.parametrize("cin", [32, 64])
def test_conv_forward_matches_float64_entry_by_entry(cin, B):
    """r48_conv3x3 with and without bias, without and with `stats`, against update_refs.conv3x3: y bit-equal
    to the float64 result rounded once (exact inputs; at cin = 32 and B = 129 also the one-hot stem input of
    r48_board_onehot32) or within out_bound(want, (9 cin + 2) u mag) (real inputs), the same bits with and
    without stats. The statistics buffer starts as NaN with its last 4 floats 0: afterwards all 256
    records are finite, those of workgroups without a tile are exactly 0, the last 4 floats are still 0
    bits, and per channel the float64 sum of the records is within (32 T + 11) u sum |y| (sum y^2) of the
    float64 sum (of squares) of the kernel's own y -- exactly equal where sum |y| / 2^-5 (sum y^2 / 2^-10)
    stays below 2^24 with exact inputs."""
    top = {}
    for kind in kinds(B, CONV_REAL) + (["onehot"] if (cin, B) == (32, 129) else []):
        forward_case(kind, B, cin, top)
    report_all("conv forward cin=%d B=%d" % (cin, B), top)


# ------------------------------------------------------------------------------- 2. data gradient
def grad_inputs(kind, B, seed):
    """dy, add, bn_x bf16 [B, 16, 64], add_mask and bn_mask [16 B, 8] with the planted columns, save fp32
    [128] = (mean: k / 4 with exact inputs, else N(0, 1) in range; invstd in [0.5, 1.5])."""
    g = gen(seed)
    dy, add, bn_x = (act(kind, (B, 16, 64), g) for _ in range(3))
    am, bm = random_mask(16 * B, g), random_mask(16 * B, g)
    if kind == "exact":
        mean = torch.randint(-8, 9, (64,), generator=g, device=DEV).float() / 4
    else:
        mean = in_range(torch.randn(64, generator=g, device=DEV))
    save = torch.cat([mean, torch.rand(64, generator=g, device=DEV) + 0.5]).contiguous()
    return Kept(dy=dy, add=add, bn_x=bn_x, add_mask=am, bn_mask=bm, save=save, w=frags(kind, 64, True))


def bn_grad(k, B, add, add_mask, fin=None, part=None):
    """r48_conv3x3_bn_grad into a guarded dx and (unless given) a fresh statistics buffer -> dx bits, raw, part."""
    t = k.t
    raw, dx = guarded(B, torch.int16, 0x5555, row=1024)
    rp, part = new_stats() if part is None else part
    check(lib().r48_conv3x3_bn_grad(ptr(t["dy"]), B, ptr(t["w"]), ptr(add), ptr(add_mask), ptr(dx), ptr(t["bn_x"]),
                                    ptr(t["bn_mask"]), ptr(t["save"]), ptr(part), None if fin is None else C.byref(fin),
                                    stream()))
    torch.cuda.synchronize()
    assert guard_ok(raw, B * 1024, 0x5555), "r48_conv3x3_bn_grad wrote past dx"
    return dx, rp, part


def grad_records_ratio(rec, k, dx, B, kind, name):
    """The records of SM = 2 against the sums of g = dx . mask bit and g (bn_x - mean) over the kernel's own dx."""
    t = k.t
    passed = mask_bool(t["bn_mask"])
    gq = torch.where(passed, dx.view(BF).double().reshape(-1, 64), 0.0)
    xc = t["bn_x"].double().reshape(-1, 64) - t["save"][:64].double()
    K = 32 * tiles_per_wave(B) + 3 + 8
    r = records_ratio(rec, gq, gq * xc, K, K + 1, None if kind == "real" else (2.0 ** -5, 2.0 ** -7), name)
    got = rec.astype(np.float64).sum(0)
    assert (got[:, ALL0] == 0).all(), "%s: a channel whose mask bits are all 0 sums nothing" % name
    assert got[0, LASTBIT] == float(gq[-1, LASTBIT]), "%s: the last row's bit alone" % name
    return r


@pytest.mark.parametrize("B", CONV_BOARDS)
def test_conv_data_gradient_matches_float64_entry_by_entry(B):
    """The data gradient (pack_conv_dgrad fragments) against update_refs.conv3x3_dgrad: r48_conv3x3 without
    add, with add, and with the masked add written out (+0 where the bit is 0; the reference masks in
    float64) -- dx bit-equal (exact inputs) or within out_bound(want, (9 x 64 + 2) u mag) (real inputs);
    r48_conv3x3_bn_grad without add, with add and with add + add_mask gives the bits of those three, and its
    records are within (32 T + 11) u sum |g| and (32 T + 12) u sum |g| |bn_x - mean| (one more rounding: the
    fp32 bn_x - mean) of the float64 sums over the kernel's own dx, exact with exact inputs (means k / 4).
    Both masks carry the planted columns: every bit 0 (its sums are exactly 0), every bit 1, and only the
    last live board's last cell (its sum g is that one entry of dx)."""
    top = {}
    for kind in kinds(B, CONV_REAL):
        k = grad_inputs(kind, B, 11 * B + (kind == "real"))
        t = k.t
        w = weights(kind, 64)[0].double()
        ab = mask_bool(t["add_mask"]).reshape(B, 16, 64)
        masked = torch.where(ab, t["add"], torch.zeros((), dtype=BF, device=DEV))
        forms = (("none", None, None, None), ("add", t["add"], t["add"], None), ("mask", masked, t["add"], t["add_mask"]))
        for form, plain_add, add, add_mask in forms:
            name = "conv dgrad %s B=%d add=%s" % (kind, B, form)
            ref_add = None if plain_add is None else torch.where(ab, t["add"].double(), 0.0) if form == "mask" else add.double()
            want, mag = U.conv3x3_dgrad(t["dy"].double(), w, ref_add)
            dx = conv(t["dy"], B, 64, t["w"], None, plain_add, None)
            merge(top, {"dx": check_bf16(kind, dx, want, mag, 9 * 64 + 2, 2.0 ** -5, name)})
            del want, mag
            dxg, rp, part = bn_grad(k, B, add, add_mask)
            assert torch.equal(dxg, dx), "%s: r48_conv3x3_bn_grad's dx differs from the plain launch's" % name
            rec = stats_records(rp, part, B)
            merge(top, grad_records_ratio(rec, k, dxg, B, kind, name), "records ")
        assert k.unchanged()
    report_all("conv dgrad B=%d" % B, top)


# ---------------------------------------------------------------------------------- 3. the folded BN
def bn_in_inputs(kind, B, seed):
    """x, res bf16 [B, 16, 64], coef fp32 [128] = (a = k / 16 with |k| <= 48, b) with the planted channels
    1: a = 1, b = 2.75, x = -2.75 (v = +0); 2: a = -1, b = -0.5, x = |x| (v < 0); 3: a = 1, b = -0, x = -0 (v = -0)."""
    g = gen(seed)
    x, res = act(kind, (B, 16, 64), g), act(kind, (B, 16, 64), g)
    a = torch.randint(-48, 49, (64,), generator=g, device=DEV).float() / 16
    if kind == "exact":
        b = torch.randint(-32, 33, (64,), generator=g, device=DEV).float() / 4
    else:
        b = in_range(torch.randn(64, generator=g, device=DEV))
    x[:, :, 1], x[:, :, 2], x[:, :, 3] = -2.75, x[:, :, 2].abs(), -0.0
    a[1], b[1], a[2], b[2], a[3], b[3] = 1.0, 2.75, -1.0, -0.5, 1.0, -0.0
    return Kept(x=x, res=res, coef=torch.cat([a, b]).contiguous(), w=frags(kind, 64), bias=weights(kind, 64)[1])


def bn_in(k, B, with_res, fin=None, stats=None):
    """r48_conv3x3_bn_in into guarded z_out, mask_out, y and a fresh (or the given) statistics buffer."""
    t = k.t
    rz, z = guarded(B, torch.int16, 0x5555, row=1024)
    rm, m = guarded(16 * B, torch.uint8, 0x55, row=8)
    ry, y = guarded(B, torch.int16, 0x5555, row=1024)
    rs, st = new_stats() if stats is None else stats
    check(lib().r48_conv3x3_bn_in(ptr(t["x"]), B, ptr(t["w"]), ptr(t["bias"]), ptr(t["coef"]), ptr(t["res"]) if with_res else None,
                                  ptr(z), ptr(m), ptr(y), ptr(st), None if fin is None else C.byref(fin), stream()))
    torch.cuda.synchronize()
    assert guard_ok(rz, B * 1024, 0x5555) and guard_ok(rm, B * 128, 0x55) and guard_ok(ry, B * 1024, 0x5555), \
        "r48_conv3x3_bn_in wrote past z_out, mask_out or y at B = %d" % B
    return z, m, y, rs, st


def open_zero(bits16):
    return torch.where(bits16 == -32768, 0, bits16)


@pytest.mark.parametrize("B", CONV_BOARDS)
@pytest.mark.parametrize("with_res", [False, True])
def test_conv_bn_in_equals_bn_apply_then_conv(with_res, B):
    """r48_conv3x3_bn_in (IN = 1, and IN = 2 with the residual): z_out and mask_out bit-equal to
    r48_bn_apply of the same x, coefficients and residual, and z_out to the float64 statement -- a = k / 16,
    so a x + b is exact in float64 and rounds once to the fused multiply-add's fp32 value; the residual is
    one fp32 add, the ReLU max(v, 0), the result rounds to nearest even bf16 (a zero's sign left open).
    Every mask byte equals the bits of z > 0; without a residual the planted channels v = +0, v < 0 and
    v = -0 set no bit. y and the 256 statistics records are bit-equal to r48_conv3x3(z, stats), the
    statistics buffers as in the forward test; with a finish (fin) z, the mask, y and the records keep
    their bits and the arrival counter is back at 0. Guards behind z_out, mask_out and y at every size:
    the clamped lanes of a ragged tile must store nothing."""
    for kind in kinds(B, CONV_REAL):
        k = bn_in_inputs(kind, B, 13 * B + with_res + 2 * (kind == "real"))
        t = k.t
        name = "conv bn_in %s B=%d res=%d" % (kind, B, with_res)
        z, m, y, rs, st = bn_in(k, B, with_res)
        rec = stats_records(rs, st, B)
        rz, za = guarded(B, torch.int16, 0x5555, row=1024)
        rk, ma = guarded(16 * B, torch.uint8, 0x55, row=8)
        check(lib().r48_bn_apply(ptr(t["x"]), ptr(t["res"]) if with_res else None, 16 * B, 64, ptr(t["coef"]), 1, ptr(za),
                                 ptr(ma), stream()))
        torch.cuda.synchronize()
        assert guard_ok(rz, B * 1024, 0x5555) and guard_ok(rk, B * 128, 0x55)
        assert torch.equal(z, za), "%s: z_out differs from r48_bn_apply's output" % name
        assert torch.equal(m, ma), "%s: mask_out differs from r48_bn_apply's mask" % name
        a, b = t["coef"][:64].double(), t["coef"][64:].double()
        v = (a * t["x"].double() + b).float()
        if with_res:
            v = v + t["res"].float()
        v = torch.where(v > 0, v, torch.zeros_like(v))
        assert torch.equal(open_zero(i16(z)), open_zero(i16(v.to(BF)))), "%s: z_out differs from the float64 statement" % name
        assert torch.equal(m, mask_of(z.view(16 * B, 64))), "%s: a mask byte is not the bits of z > 0" % name
        if not with_res:
            assert not bool(mask_bool(m)[:, 1:4].any()) and bool((z.view(-1, 64)[:, 1:4] == 0).all())
        rs2, st2 = new_stats()
        y2 = conv(z.view(BF).view(B, 16, 64), B, 64, t["w"], t["bias"], None, st2)
        assert torch.equal(y, y2), "%s: y differs from r48_conv3x3 of z" % name
        assert (rec.view(np.int32) == stats_records(rs2, st2, B).view(np.int32)).all(), "%s: the records differ" % name
        gamma, beta = bn_params(gen(B))[:2]
        save, coef = torch.empty(128, device=DEV), torch.empty(128, device=DEV)
        fin = fin_args(gamma, beta, None, None, save, coef, None, None, 16 * B, 0.1, 1e-5)
        zf, mf, yf, rsf, stf = bn_in(k, B, with_res, fin=fin)
        assert torch.equal(zf, z) and torch.equal(mf, m) and torch.equal(yf, y), "%s: the finish changes an output" % name
        assert (stats_records(rsf, stf, B).view(np.int32) == rec.view(np.int32)).all()
        assert k.unchanged()
    print("conv bn_in B=%d res=%d: worst error / bound: bit-exact 0" % (B, with_res))


# ------------------------------------------------------------------------------ 4. the finishing forms
def bn_params(g):
    gamma = torch.randn(64, generator=g, device=DEV) * 0.5 + 1.0
    beta, rm = torch.randn(64, generator=g, device=DEV), torch.randn(64, generator=g, device=DEV)
    return gamma, beta, rm, torch.rand(64, generator=g, device=DEV) + 0.5


def forward_finish_ratio(rec, rows, gamma, beta, rm, rv, momentum, eps, save, coef, run, running):
    """save, coef and the running statistics of a forward finish against update_refs.bn_from_sums of the
    float64 sum of the kernel's own records, within fwd_bounds with the record-sum terms of
    test_bn_record_forms_match_float64_of_the_same_records."""
    r64 = rec.astype(np.float64)
    s, mag = r64.sum(0), np.abs(r64).sum(0)
    h64 = lambda v: host(v).astype(np.float64)      # noqa: E731
    f = U.bn_from_sums(s[0], s[1], rows, 0.0, h64(gamma), h64(beta), h64(rm) if running else None,
                       h64(rv) if running else None, momentum, eps)
    e_dm = TFIN * mag[0] / rows
    e_var = TFIN * mag[1] / rows + 2 * np.abs(f["mean"]) * e_dm + 4 * D53 * (s[1] / rows + f["mean"] ** 2)
    e = fwd_bounds(f, rows, e_dm, e_var, host(gamma), eps, momentum)
    sv, cf, rn = host(save), host(coef), host(run)
    r = {"mean": worst(np.abs(sv[:64] - f["mean"]), e["mean"]), "invstd": worst(np.abs(sv[64:] - f["invstd"]), e["invstd"]),
         "a": worst(np.abs(cf[:64] - f["a"]), e["a"]), "b": worst(np.abs(cf[64:] - f["b"]), e["b"])}
    if running:
        r["rm"] = worst(np.abs(rn[:64] - f["rm"]), e["rm"])
        r["rv"] = worst(np.abs(rn[64:] - f["rv"]), e["rv"])
    else:
        assert (rn == 7.5).all(), "no running statistics were given"
    return r


@pytest.mark.parametrize("B", FIN_BOARDS)
@pytest.mark.parametrize("form", ["stats_finish 32", "stats_finish 64", "bn_in", "bn_in res"])
def test_conv_forward_finish_matches_float64_of_its_own_records(form, B):
    """r48_conv3x3_stats_finish (cin 32 and 64) and r48_conv3x3_bn_in with fin (without and with the
    residual) at rows = 16 B (B = 1: 255 idle workgroups that still take a ticket), with running statistics
    and with both NULL: save {mean, invstd}, coef {a, b} and the running statistics against
    update_refs.bn_from_sums of the float64 sum of the kernel's own fp32 records, within fwd_bounds (each
    output one float64 expression cast once; TFIN of the summed magnitudes for the order of the float64
    sums). The statistics buffer starts as NaN with the counter and its pad 0: afterwards the records are
    finite (idle ones 0), the counter is 0 bits and the pad untouched; y has the bits of the form without a
    finish. A second call on the same buffer, not zeroed again, gives the same bits everywhere."""
    top = {}
    cin = 32 if form.endswith("32") else 64
    for kind in ("exact", "real"):
        for running in (True, False):
            g = gen(17 * B + cin + running + 2 * (kind == "real"))
            momentum, eps = (f32(v) for v in MOM_EPS[(B + running) % 6])
            gamma, beta, rm0, rv0 = bn_params(g)
            if form.startswith("bn_in"):
                k = bn_in_inputs(kind, B, 19 * B + (kind == "real"))
            else:
                k = Kept(x=act(kind, (B, 16, cin), g), w=frags(kind, cin), bias=weights(kind, cin)[1])
            kp = Kept(gamma=gamma, beta=beta)
            stats = new_stats()
            outs = []
            for _ in range(2):
                rsv, save = guarded(128, torch.float32, 7.5)
                rcf, coef = guarded(128, torch.float32, 7.5)
                rrn, run = guarded(128, torch.float32, 7.5)
                if running:
                    run.copy_(torch.cat([rm0, rv0]))
                fin = fin_args(gamma, beta, run[:64] if running else None, run[64:] if running else None, save, coef, None,
                               None, 16 * B, momentum, eps)
                if form.startswith("bn_in"):
                    z, m, y, _, _ = bn_in(k, B, form.endswith("res"), fin=fin, stats=stats)
                    plain = bn_in(k, B, form.endswith("res"))[2]
                else:
                    ry, y = guarded(B, torch.int16, 0x5555, row=1024)
                    check(lib().r48_conv3x3_stats_finish(ptr(k.t["x"]), B, cin, ptr(k.t["w"]), ptr(k.t["bias"]), ptr(y),
                                                         ptr(stats[1]), C.byref(fin), stream()))
                    torch.cuda.synchronize()
                    assert guard_ok(ry, B * 1024, 0x5555)
                    plain = conv(k.t["x"], B, cin, k.t["w"], k.t["bias"], None, None)
                assert torch.equal(y, plain), "%s: the finish changes y" % form
                rec = stats_records(*stats, B)
                assert guard_ok(rsv, 128, 7.5) and guard_ok(rcf, 128, 7.5) and guard_ok(rrn, 128, 7.5)
                outs.append([y.clone(), stats[1].clone(), save.clone(), coef.clone(), run.clone()])
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*outs)), \
                "%s: a second call on the same statistics buffer gives other bits" % form
            merge(top, forward_finish_ratio(rec, 16 * B, gamma, beta, rm0, rv0, momentum, eps, save, coef, run, running))
            assert k.unchanged() and kp.unchanged()
    report_all("conv forward finish %s B=%d" % (form, B), top)


@pytest.mark.parametrize("B", FIN_BOARDS)
@pytest.mark.parametrize("form", ["none", "add", "mask"])
def test_conv_bn_grad_finish_matches_float64_of_its_own_records(form, B):
    """r48_conv3x3_bn_grad with fin at rows = 16 B, with dgamma / dbeta and with both NULL: dgamma, dbeta and
    coef {a, cc, d} against update_refs.bn_backward_from_sums of the float64 sum of the kernel's own fp32
    records (mean and invstd the fp32 save, exactly), within bwd_bounds (save_exact; TFIN of the summed
    magnitudes for the order of the float64 sums). dx has the bits of the form without a finish; records,
    counter, pad and the second call as in the forward finish."""
    top = {}
    for kind in ("exact", "real"):
        for with_grads in (True, False):
            k = grad_inputs(kind, B, 23 * B + with_grads + 2 * (kind == "real"))
            t = k.t
            gamma = bn_params(gen(B))[0]
            kp = Kept(gamma=gamma)
            add = None if form == "none" else t["add"]
            add_mask = t["add_mask"] if form == "mask" else None
            stats = new_stats()
            outs = []
            for _ in range(2):
                rcf, coef = guarded(192, torch.float32, 7.5)
                rgr, grads = guarded(128, torch.float32, 7.5)
                fin = fin_args(gamma, None, None, None, t["save"], coef, grads[:64] if with_grads else None,
                               grads[64:] if with_grads else None, 16 * B, 0.0, 0.0)
                dx, _, _ = bn_grad(k, B, add, add_mask, fin=fin, part=stats)
                assert torch.equal(dx, bn_grad(k, B, add, add_mask)[0]), "the finish changes dx"
                rec = stats_records(*stats, B)
                assert guard_ok(rcf, 192, 7.5) and guard_ok(rgr, 128, 7.5)
                outs.append([dx.clone(), stats[1].clone(), coef.clone(), grads.clone()])
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*outs)), \
                "a second call on the same statistics buffer gives other bits"
            r64 = rec.astype(np.float64)
            s, mag = r64.sum(0), np.abs(r64).sum(0)
            sv = host(t["save"]).astype(np.float64)
            mean, invstd = sv[:64], sv[64:]
            b = U.bn_backward_from_sums(s[0], s[1], 16 * B, mean, invstd, host(gamma).astype(np.float64))
            e = bwd_bounds(b, 16 * B, 64, mean, invstd, TFIN * mag[0], TFIN * mag[1], True)
            cf, gr = host(coef), host(grads)
            r = {"a": worst(np.abs(cf[:64] - b["a"]), e["a"]), "cc": worst(np.abs(cf[64:128] - b["cc"]), e["cc"]),
                 "d": worst(np.abs(cf[128:] - b["d"]), e["d"])}
            if with_grads:
                r["dgamma"] = worst(np.abs(gr[:64] - b["dgamma"]), e["dgamma"])
                r["dbeta"] = worst(np.abs(gr[64:] - b["dbeta"]), e["dbeta"])
                assert gr[ALL0] == 0 and gr[64 + ALL0] == 0, "a channel whose mask bits are all 0"
            else:
                assert (gr == 7.5).all(), "no dgamma / dbeta were given"
            merge(top, r)
            assert k.unchanged() and kp.unchanged()
    report_all("conv bn_grad finish add=%s B=%d" % (form, B), top)


# ------------------------------------------------------------------------------ 5. the weight gradient
def wgrad(dy, x, B, cin, finite=True):
    """r48_conv3x3_wgrad twice into guarded, poisoned dw and workspace (NaN) -> dw [64, cin, 3, 3] (host)."""
    n = int(lib().r48_conv_wgrad_workspace_floats(cin))
    assert n == (NREC + 16) * 9 * 64 * cin
    outs = []
    for _ in range(2):
        rw, ws = guarded(n, torch.float32, 7.5)
        ws.fill_(float("nan"))
        rd, dw = guarded(64 * cin * 9, torch.float32, 7.5)
        check(lib().r48_conv3x3_wgrad(ptr(dy), ptr(x), B, cin, ptr(ws), ptr(dw), stream()))
        torch.cuda.synchronize()
        assert guard_ok(rw, n, 7.5) and guard_ok(rd, 64 * cin * 9, 7.5), "r48_conv3x3_wgrad wrote past its workspace or dw"
        assert not finite or bool(torch.isfinite(ws[:NREC * 9 * 64 * cin]).all()), "a workgroup left its record unwritten"
        outs.append((dw.clone(), ws[:NREC * 9 * 64 * cin].clone()))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), "a second call gives other bits"
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)), "a second call gives other records"
    return host(outs[0][0]).reshape(64, cin, 3, 3)


def wgrad_K(B, cin):
    ksplit = 128 // cin
    steps = -(-16 * B // 128)
    return 32 * (4 // ksplit) * -(-steps // NREC) + (ksplit - 1) + 32


@pytest.mark.parametrize("B", WGRAD_BOARDS)
@pytest.mark.parametrize("cin", [32, 64])
def test_conv_wgrad_matches_float64_entry_by_entry(cin, B):
    """r48_conv3x3_wgrad against update_refs.conv3x3_wgrad, all 64 x cin x 9 entries: equal to the float64
    result itself with exact inputs (sum |terms| / 2^-4 < 2^24 up to 6,160 boards, asserted) -- random ones;
    every row of dy and x zero but the LAST live row (the whole gradient is one outer product, in the
    centre tap: a ragged step that loses or repeats its last real row cannot hide); only the FIRST row
    non-zero; and random ones with +inf in one channel of x's last live row -- a ragged step stages its rows
    past the end from that (clamped) row and must zero them in BOTH images: dy's zeros times a copy of the
    inf would be NaN, so the entries that float64 leaves finite (every tap that does not read the last cell,
    every other channel) stay finite and exact, the others are not finite in both -- and within K u mag +
    u |want| with real inputs, K = 32 kPer ceil(steps / 256) + (kSplit - 1) + 32. The workspace (r48_conv_wgrad_workspace_floats(cin), NaN) and dw are guarded; all 256 records are
    finite afterwards; a second call gives the same bits."""
    top = {}
    g = gen(29 * B + cin)
    cases = []
    for kind in kinds(B, WGRAD_REAL):
        cases.append((kind, act(kind, (B, 16, 64), g), act(kind, (B, 16, cin), g)))
    for which, row in (("last row", 16 * B - 1), ("first row", 0)):
        dy, x = torch.zeros(16 * B, 64, device=DEV), torch.zeros(16 * B, cin, device=DEV)
        for t in (dy, x):
            v = torch.randint(1, 5, (t.shape[1],), generator=g, device=DEV).float() / 4
            t[row] = torch.where(torch.rand(t.shape[1], generator=g, device=DEV) < 0.5, -v, v)
        cases.append((which, dy.to(BF).view(B, 16, 64), x.to(BF).view(B, 16, cin)))
    dy, x = act("exact", (B, 16, 64), g), act("exact", (B, 16, cin), g)
    x[B - 1, 15, 3] = float("inf")
    cases.append(("inf", dy, x))
    for kind, dy, x in cases:
        name = "conv wgrad %s B=%d cin=%d" % (kind, B, cin)
        k = Kept(dy=dy, x=x)
        want, mag = (host(v) for v in U.conv3x3_wgrad(dy.double(), x.double()))
        got = wgrad(dy, x, B, cin, finite=kind != "inf")
        assert k.unchanged()
        if kind == "inf":
            fin = np.isfinite(want)
            assert fin[:, :, 0, :].all() and fin[:, :3].all() and not fin[:, 3, 1, 1].any(), "the reference's own inf"
            assert (np.isfinite(got) == fin).all(), "%s: %d entries are not finite where float64 is (or the reverse)" % (
                name, (np.isfinite(got) != fin).sum())
            assert (got[fin] == want[fin].astype(F32)).all() and mag[fin].max() / 2.0 ** -4 < 2.0 ** 24
            merge(top, {"exact": 0.0})
            continue
        assert not np.isnan(got).any()
        if kind == "real":
            r = worst(np.abs(got.astype(np.float64) - want), (wgrad_K(B, cin) * u * mag + u * np.abs(want)) * SLACK)
            assert r <= 1, "%s: %.3g of the bound" % (name, r)
            merge(top, {"dw": r})
            continue
        assert multiple_of(dy, 0.25) and multiple_of(x, 0.25) and mag.max() / 2.0 ** -4 < 2.0 ** 24
        bad = got != want.astype(F32)
        assert not bad.any(), "%s: %d entries differ from float64, the first at (co, ci, kr, kc) = %r" % (
            name, bad.sum(), tuple(np.argwhere(bad)[0]))
        if kind in ("last row", "first row"):
            centre = np.outer(host(dy.float().view(-1, 64))[16 * B - 1 if kind == "last row" else 0],
                              host(x.float().view(-1, cin))[16 * B - 1 if kind == "last row" else 0])
            assert (got[:, :, 1, 1] == centre).all() and np.count_nonzero(got) == centre.size
        merge(top, {"exact": 0.0})
    report_all("conv wgrad cin=%d B=%d" % (cin, B), top)


# ------------------------------------------------------------------------------ 6. argument checks
def test_conv_entries_refuse_bad_arguments_and_write_nothing():
    """R48_EINVAL without a launch from r48_conv3x3, r48_conv3x3_stats_finish, r48_conv3x3_bn_in,
    r48_conv3x3_bn_grad and r48_conv3x3_wgrad: cin = 48, boards = 0, each pointer that all_aligned16 checks
    2 bytes off, add with cin 32 or with stats, add_mask without add, fin->save != bn_save, one running
    statistic without the other, an incomplete fin, and each required pointer NULL. Every output buffer
    keeps its poison."""
    from rein48_amd import _lib
    B = 3
    L, s, bad = lib(), stream(), _lib.R48_EINVAL
    k = grad_inputs("exact", B + 1, 5)
    t = k.t
    x32 = act("exact", (B + 1, 16, 32), gen(6))
    fr, fr32, bias = frags("exact", 64), frags("exact", 32), weights("exact", 64)[1]
    coef_in = torch.cat([torch.ones(64, device=DEV), torch.zeros(64, device=DEV)])
    kin = Kept(x32=x32, fr=fr, fr32=fr32, bias=bias, coef_in=coef_in)
    outs = [torch.full((B + 1, 1024), 0x5555, dtype=torch.int16, device=DEV) for _ in range(2)]
    y, z = outs
    mk = torch.full((16 * (B + 1), 8), 0x55, dtype=torch.uint8, device=DEV)
    nws = int(L.r48_conv_wgrad_workspace_floats(64))
    fl = [torch.full((n,), 7.5, dtype=torch.float32, device=DEV) for n in (NREC * 128 + 4, 256, 256, 256, nws, 64 * 64 * 9)]
    st, save, coef, run, ws, dw = fl
    gamma = torch.ones(64, device=DEV)

    def off(tensor):
        return C.c_void_p(tensor.data_ptr() + 2)

    def fin(**kw):
        a = dict(gamma=gamma, beta=gamma, rm=None, rv=None, save=save, coef=coef, dgamma=None, dbeta=None, rows=16 * B)
        a.update(kw)
        return C.byref(fin_args(a["gamma"], a["beta"], a["rm"], a["rv"], a["save"], a["coef"], a["dgamma"], a["dbeta"],
                                a["rows"], 0.1, 1e-5))

    def a(d, **kw):
        d = dict(d)
        d.update(kw)
        return d

    def p(v):
        return v if isinstance(v, C.c_void_p) or v is None or not torch.is_tensor(v) else ptr(v)

    def conv_(**kw):
        d = a(dict(x=t["dy"], n=B, cin=64, w=fr, bias=bias, add=None, y=y, st=None), **kw)
        return L.r48_conv3x3(p(d["x"]), d["n"], d["cin"], p(d["w"]), p(d["bias"]), p(d["add"]), p(d["y"]), p(d["st"]), s)

    def sfin(**kw):
        d = a(dict(x=t["dy"], n=B, cin=64, w=fr, bias=bias, y=y, st=st, fin=fin()), **kw)
        return L.r48_conv3x3_stats_finish(p(d["x"]), d["n"], d["cin"], p(d["w"]), p(d["bias"]), p(d["y"]), p(d["st"]), d["fin"], s)

    def bnin(**kw):
        d = a(dict(x=t["dy"], n=B, w=fr, bias=bias, coef=coef_in, res=None, z=z, m=mk, y=y, st=st, fin=None), **kw)
        return L.r48_conv3x3_bn_in(p(d["x"]), d["n"], p(d["w"]), p(d["bias"]), p(d["coef"]), p(d["res"]), p(d["z"]), p(d["m"]),
                                   p(d["y"]), p(d["st"]), d["fin"], s)

    def bngr(**kw):
        d = a(dict(dy=t["dy"], n=B, w=t["w"], add=None, am=None, dx=y, bx=t["bn_x"], bm=t["bn_mask"], sv=t["save"], part=st,
                   fin=None), **kw)
        return L.r48_conv3x3_bn_grad(p(d["dy"]), d["n"], p(d["w"]), p(d["add"]), p(d["am"]), p(d["dx"]), p(d["bx"]), p(d["bm"]),
                                     p(d["sv"]), p(d["part"]), d["fin"], s)

    def wg(**kw):
        d = a(dict(dy=t["dy"], x=t["bn_x"], n=B, cin=64, ws=ws, dw=dw), **kw)
        return L.r48_conv3x3_wgrad(p(d["dy"]), p(d["x"]), d["n"], d["cin"], p(d["ws"]), p(d["dw"]), s)
    NULL = None
    bfin = dict(beta=None, save=t["save"])          # a backward finish reads bn_save
    calls = {
        "cin = 48": [conv_(cin=48), sfin(cin=48), wg(cin=48)],
        "boards = 0": [conv_(n=0), sfin(n=0), bnin(n=0), bngr(n=0), wg(n=0)],
        "2 bytes off": [conv_(x=off(t["dy"])), conv_(w=off(fr)), conv_(y=off(y)), conv_(bias=off(bias)), conv_(add=off(t["add"])),
                        sfin(x=off(t["dy"])), sfin(w=off(fr)), sfin(y=off(y)), sfin(bias=off(bias)),
                        bnin(x=off(t["dy"])), bnin(w=off(fr)), bnin(y=off(y)), bnin(bias=off(bias)), bnin(coef=off(coef_in)),
                        bnin(res=off(t["add"])), bnin(z=off(z)),
                        bngr(dy=off(t["dy"])), bngr(w=off(t["w"])), bngr(dx=off(y)), bngr(add=off(t["add"])),
                        bngr(bx=off(t["bn_x"])), bngr(sv=off(t["save"])),
                        wg(dy=off(t["dy"])), wg(x=off(t["bn_x"])), wg(ws=off(ws))],
        "add with cin 32 or stats": [conv_(x=x32, cin=32, w=fr32, add=t["add"]), conv_(add=t["add"], st=st)],
        "add_mask without add": [bngr(am=t["add_mask"])],
        "fin->save != bn_save": [bngr(fin=fin(beta=None)), bngr(fin=fin(beta=None, save=t["save"][64:]))],
        "one running statistic": [sfin(fin=fin(rm=run)), sfin(fin=fin(rv=run)), bnin(fin=fin(rm=run)), bnin(fin=fin(rv=run))],
        "an incomplete fin": [sfin(fin=NULL), sfin(fin=fin(gamma=None)), sfin(fin=fin(beta=None)), sfin(fin=fin(save=None)),
                              sfin(fin=fin(coef=None)), sfin(fin=fin(rows=0)),
                              bnin(fin=fin(gamma=None)), bnin(fin=fin(beta=None)), bnin(fin=fin(save=None)),
                              bnin(fin=fin(coef=None)), bnin(fin=fin(rows=0)),
                              bngr(fin=fin(gamma=None, **bfin)), bngr(fin=fin(coef=None, **bfin)), bngr(fin=fin(rows=0, **bfin))],
        "a NULL pointer": [conv_(x=NULL), conv_(w=NULL), conv_(y=NULL),
                           sfin(x=NULL), sfin(w=NULL), sfin(y=NULL), sfin(st=NULL),
                           bnin(x=NULL), bnin(w=NULL), bnin(coef=NULL), bnin(z=NULL), bnin(m=NULL), bnin(y=NULL), bnin(st=NULL),
                           bngr(dy=NULL), bngr(w=NULL), bngr(dx=NULL), bngr(bx=NULL), bngr(bm=NULL), bngr(sv=NULL), bngr(part=NULL),
                           wg(dy=NULL), wg(x=NULL), wg(ws=NULL), wg(dw=NULL)],
    }
    for what, codes in calls.items():
        assert all(code == bad for code in codes), "%s: %r" % (what, codes)
    assert L.r48_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 0x5555).all()) for o in outs) and all(bool((v == 7.5).all()) for v in fl)
    assert bool((mk == 0x55).all()) and k.unchanged() and kin.unchanged()
