"""The four GEMM kernels (K3 gemm_nt_kernel, K3s gemm_skinny_kernel, K3d gemm_8p_kernel, K3w
gemm_ws_kernel), one launch at a time through mrag_gemm_nt / mrag_gemm_nt_kernel / mrag_gemm_nt_ld,
at the shapes where their pipelines change branch, into guarded buffers, against

  (a) the exact result: integer operands whose every partial sum is an integer below 2^24, so the
      f32 result is exact in any accumulation order (R.gemm_int_operands), and
  (b) a float64 reference per element, with a derived bound, on real-valued operands: plain ones
      with outlier columns, and ones whose dot products cancel (|x| << S), where the max-norm
      comparison of tests/test_encoders_gpu.py sees nothing.

References and generators: tests/_kernel_refs.py (checked on the CPU by test_kernel_refs_cpu.py).

The per-element bound. S = |A| |W|^T + |bias| (+ |C0|). The accumulator: |acc - x| <= ACC(S) =
(K + K / 32 + 2) 2^-23 S (R.gemm_acc_bound): the K products are exact in f32, and they, the K / 32
MFMA chunk results, the bias and C0 are summed with at most one rounding each. The one assumption
about the MFMA's internals is the proviso of that bound: every intermediate of a 32-deep chunk
keeps at least f32 precision (an error of at most 2^-23 relative per addition) under whatever
rounding mode and summation order the hardware uses. Per epilogue:
  4, 3:  ACC
  0:     ACC + 2^-11 |ref| + 2^-25             (fp16 rounding; 2^-25: half a subnormal step)
  1, 2:  1.13 ACC + ACT(ref) + 2^-11 |ref| + 2^-25
1.13 bounds the slope of both activations (test_gemm_activation_slopes); ACT is the error of
gemm_act's own evaluation at an exact argument, from its code (csrc/encoder_kernels.hip):
  quick-GELU  y = x * rcp(1 + exp2(c x)), c = f32(-1.702 f32(log2 e)). The exp2 argument carries
    the roundings of 1.702, log2 e, their product and c x: <= 2^-22 relative, i.e. 2^-22 |c x| ln 2
    relative in exp2's result, plus exp2's own ulp (2^-23): the sigmoid s moves by s (1 - s) times
    that, y by |x| s (1 - s) (2^-22 ln 2 |c x| + 2^-23). With u = 1.702 x, u^2 s (1 - s) <= 0.44 and
    |u| (1 - s) <= 0.28: <= 0.26 2^-22 + 0.17 2^-23 = 8.2e-8 absolute. The addition 1 + e (2^-24),
    rcp (one ulp, 2^-23) and the product (2^-24) are relative to y: 2^-22 |y|.
    QGELU_ABS = 1e-7, ACT_REL = 2^-21 (twice the relative part).
  erf-GELU    the project's figure (gemm_act's comment, test_gelu_erf_epilogue_sweep): the A&S
    7.1.26 error 1.5e-7 gives 0.5 |x| 1.5e-7, at most 4.5e-7 before e saturates at |x| ~ 6, plus
    rcp / exp2 ulps: GELU_ERF_ABS = 2e-6, and the same ACT_REL for the products relative to y.

Every launch goes through guarded_launch: C is rows [0, M), columns [0, N) of a buffer of M + 256
rows with ldc = N + 8 (and ldc = N, what the towers pass), pre-filled with NaN (C0 for epilogue 3)
inside and a fixed byte pattern in the guard rows and pad columns; A is the first M rows of a
buffer with 64 more rows of NaN. After the launch: guards unchanged byte for byte, no NaN in C,
A / W / bias unchanged, and a second launch (from the same pre-fill) gives the same bytes.
Flags and ratios stay on the device and are read back once per test.
"""
from __future__ import annotations

import pytest
import torch

import _kernel_refs as R
from conftest import record_numerics

pytestmark = pytest.mark.gpu

F16_EPS = 2.0 ** -11
SLOPE = 1.13
# Observed on MI355X, max err / bound (every figure is recorded and printed in the numerics section):
#   real operands, f32 epilogues 3 / 4 (the ACC term alone): K3 0.0097 / 0.0105, K3s 0.0039 / 0.0042,
#     K3d 0.0109 / 0.0116; cancelling operands against ACC: 0.0010 - 0.0027
#   real operands, f16 epilogues 0 / 1 / 2: K3 0.913 / 0.901 / 0.902, K3s 0.756 / 0.736 / 0.734,
#     K3d 0.914 / 0.906 / 0.904, K3w 0.829 / 0.812 / 0.812 (a half-ulp fp16 rounding reaches its term)
#   integer operands (acc exact), epilogues 1 / 2 at K = 64: 0.25 / 0.15 (ACT + fp16 rounding alone)
#   past-INT_MAX batch through the rule (K = 3072, epilogue 0): 0.099
QGELU_ABS = 1e-7     # sweep: 0.996 of the bound; max (|err| - 2^-11 |ref| - 2^-25) = -1.6e-11: the fp16 rounding alone
GELU_ERF_ABS = 2e-6  # test_gelu_erf_epilogue_sweep's figure
ACT_REL = 2.0 ** -21
GUARD_ROWS, GUARD_A_ROWS, PAD_COLS = 256, 64, 8
GUARD_BYTE = 0x5A

# K3s ring depth per activation-block count MB = ceil(M / 16): SkinnyGeom<MB>::RP in
# csrc/encoder_kernels.hip (its static_assert: (RP - 1) (2 + 2 MB) < 64, the vmcnt field)
K3S_RP = {1: 16, 2: 10, 3: 7, 4: 6}
assert all((rp - 1) * (2 + 2 * mb) < 64 for mb, rp in K3S_RP.items())

# ---- shape lists: (M, N, K, reason) ----------------------------------------------------------
K3_MS = [
    (1, "one row: 127 clamped A rows per tile, one store row"),
    (15, "ragged inside the first 16-row MFMA block"), (16, "exactly one block"), (17, "one row into block 1"),
    (63, "wave row 0 ragged"), (64, "wave row 0 full, wave row 1 without a store"), (65, "one row into wave row 1"),
    (127, "last row of the tile missing"), (128, "one full tile"), (129, "second tile with one row"),
    (255, "second tile ragged by one"), (256, "two full tiles"), (257, "third tile with one row"),
    (1000, "eight tiles, the last ragged (1000 = 7 * 128 + 104)"),
]
# N = 128: grids of 1, 2, 3 and 8 workgroups; N = 384: 3, 6, 9 and 24 (xcd_remap below 8 blocks, at 8,
# and with nwg & 7 != 0); K = 64 / 128 / 192: one, two and three k-steps (no prefetch, both stages)
K3_SHAPES = [(M, N, K, why) for N in (128, 384) for K in (64, 128, 192) for M, why in K3_MS]

K3S_SHAPES = []
for _mb, _rp in K3S_RP.items():
    _ms = sorted({1, 16 * (_mb - 1) + 1, 16 * _mb - 1, 16 * _mb})
    for _np in (1, 2, _rp - 1, _rp, _rp + 1, _rp + 2, 2 * _rp + 1):
        for _m in _ms:
            if _m == 1 and _mb > 1:
                continue
            K3S_SHAPES.append((_m, 128, 64 * _np, f"MB={_mb} RP={_rp} npairs={_np}: ring "
                               + ("not full" if _np < _rp else "exactly full" if _np == _rp else
                                  "refilled %d times" % (_np - _rp))))

K3D_MS = [
    (1024, "four full tile rows (the smallest M K3d takes)"), (1025, "a fifth tile with one row: st_cnt minimal"),
    (1039, "last 16-row block ragged"), (1040, "one block exactly"), (1041, "one row into block 1"),
    (1087, "quadrant HM = 64 ragged by one"), (1088, "one quadrant exactly"), (1089, "one row into the next quadrant"),
    (1151, "wave row WM = 128 ragged by one"), (1152, "wave row 0 full, wave row 1 stores nothing"),
    (1153, "one row into wave row 1"), (1279, "last tile ragged by one"), (1280, "five full tiles"),
]
# N = 256, K = 64 / 128 / 192: one tile per workgroup, total = 4 (the short-stream branch of
# end_reads: fewer than 7 half-tiles), 8 and 12 half-tiles
K3D_SHAPES = [(M, 256, K, why) for K in (64, 128, 192) for M, why in K3D_MS] + [
    (1100, 512, 64, "two tile columns, total = 4"),
    (1024, 4096, 64, "N = G8_BIAS_MAX: the bias staged in LDS to its last float"),
]

K3W_SHAPES = [(M, N, K, f"<NB, KT> instantiation of N={N} K={K}; " + why)
              for N, K in ((256, 512), (384, 512), (256, 384), (384, 384))
              for M, why in ((4096, "64 full tiles"), (4097, "a 65th tile with one row"),
                             (4159, "last tile ragged by one"), (4160, "65 full tiles"))] + [
    (6500, 2048, 512, "102 tiles over R = 32 row ranges: three and four tiles per workgroup (both parities)"),
    (6500, 1536, 384, "the same at NB = 3, KT = 12"),
]
K3W_FLAT_MAP = [(4133, 8448, 384, 5), (4133, 8448, 512, 7)]  # (M, N, K, R at 256 CUs): xcd_map == 0


def _accepting(M, N, K, epi):
    """The kernels whose launch rules (launch_gemm) accept the shape."""
    ks = ["k3", "auto"]
    if M <= 64:
        ks.append("k3s")
    if M >= 1024 and N % 256 == 0 and N <= 4096:
        ks.append("k3d")
    if epi <= 2 and K in (384, 512) and (N % 256 == 0 or N % 192 == 0) and M >= 4096:
        ks.append("k3w")
    return ks


# ---- helpers ---------------------------------------------------------------------------------
def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


_GUARD_WORD = {2: 0x5A5A, 4: 0x5A5A5A5A}


class _Checks:
    """Device-side pass / fail flags and err / bound ratios, read back once."""

    def __init__(self):
        self.flags, self.ratios = [], []

    def flag(self, label, what, bad):
        self.flags.append((label, what, bad.reshape(())))

    def ratio(self, key, label, r):
        self.ratios.append((key, label, torch.nan_to_num(r.reshape(()).double(), nan=float("inf"))))

    def finish(self):
        worst = {}
        if self.ratios:
            vals = torch.stack([r for _, _, r in self.ratios]).cpu().tolist()
            for (key, label, _), v in zip(self.ratios, vals):
                if key not in worst or v > worst[key][0]:
                    worst[key] = (v, label)
            for key, (v, label) in sorted(worst.items(), key=str):
                print("gemm", key, "max err / bound = %.3g" % v, "at", label)
        if self.flags:
            bad = torch.stack([b for _, _, b in self.flags]).cpu().tolist()
            failed = [(label, what) for (label, what, _), b in zip(self.flags, bad) if b]
            assert not failed, (len(failed), failed[:12])
        over = {k: v for k, v in worst.items() if not v[0] <= 1.0}
        assert not over, over
        return worst


class _Ops:
    """One set of operands on the device: A inside its guard buffer (64 NaN rows behind it), and
    the clones the unchanged-inputs check compares with."""

    def __init__(self, A, W, bias, C0, cuda):
        M, K = A.shape
        abuf = torch.full((M + GUARD_A_ROWS, K), float("nan"), dtype=torch.float16, device=cuda)
        abuf[:M] = A
        self.abuf, self.A = abuf, abuf[:M]
        self.W, self.bias, self.C0 = W.to(cuda), bias.to(cuda), (C0.to(cuda) if C0 is not None else None)
        self.keep = (abuf.clone(), self.W.clone(), self.bias.clone())
        self.lda = None

    def changed(self):
        a, w, b = self.keep
        return ((_bits(self.abuf) != _bits(a)).any() | (_bits(self.W) != _bits(w)).any()
                | (_bits(self.bias) != _bits(b)).any())


def guarded_launch(chk, label, ops, epi, kernel, use_bias=True, pad=PAD_COLS, c_init=None):
    """Two launches of one GEMM into a guarded C (module docstring); returns C [M][N] of the first
    (a view of its buffer's snapshot) and files the guard / NaN / inputs / repeat flags in chk.
    c_init: what epilogue 3 starts from instead of ops.C0."""
    from app.encoders import gemm_nt

    A, W = ops.A, ops.W
    M, N = A.shape[0], W.shape[0]
    cuda = W.device
    dt = torch.float16 if epi <= 2 else torch.float32
    ldc = N + pad
    cbuf = torch.empty((M + GUARD_ROWS, ldc), dtype=dt, device=cuda)
    word = _GUARD_WORD[cbuf.element_size()]
    bias = ops.bias if use_bias else None

    def run():
        cbuf.view(torch.uint8).fill_(GUARD_BYTE)
        if epi == R.GEMM_RESIDUAL:
            cbuf[:M, :N] = ops.C0 if c_init is None else c_init
        else:
            cbuf[:M, :N] = float("nan")
        if pad or ops.lda is not None:
            gemm_nt(A, W, bias, cbuf, epi, kernel=kernel, lda=ops.lda if ops.lda is not None else A.shape[1], ldc=ldc)
        else:
            gemm_nt(A, W, bias, cbuf, epi, kernel=kernel)  # mrag_gemm_nt / mrag_gemm_nt_kernel: ldc = N

    run()
    first = cbuf.clone()
    run()
    lab = (label, "epi", epi, kernel, "bias" if use_bias else "no bias", "ldc=N+%d" % pad)
    guard = (_bits(first[M:]) != word).any()
    if pad:
        guard = guard | (_bits(first[:M, N:]) != word).any()
    chk.flag(lab, "guard rows / pad columns written", guard)
    chk.flag(lab, "NaN left in C", torch.isnan(first[:M, :N]).any())
    chk.flag(lab, "A / W / bias modified", ops.changed())
    chk.flag(lab, "second launch differs", (_bits(first) != _bits(cbuf)).any())
    return first[:M, :N]


def gemm_bound(ref, S, K, epi):
    acc = R.gemm_acc_bound(S, K)
    if epi >= 3:
        return acc
    if epi == 0:
        return acc + F16_EPS * ref.abs() + 2.0 ** -25
    act = (QGELU_ABS if epi == R.GEMM_QUICK_GELU else GELU_ERF_ABS) + ACT_REL * ref.abs()
    return SLOPE * acc + act + F16_EPS * ref.abs() + 2.0 ** -25


def _exact_shape(chk, cuda, M, N, K, primary, seed, epis=range(5)):
    """(a) on one shape: the primary kernel with and without bias, with and without pad columns,
    every other accepting kernel with bias and pad columns; exact results, equal bytes."""
    A, W, bias, C0 = R.gemm_int_operands(M, N, K, seed, device=cuda)
    ops = _Ops(A, W, bias, C0, cuda)
    shape = (M, N, K)
    for epi in epis:
        kernels = _accepting(M, N, K, epi)
        if primary not in kernels:
            continue
        for use_bias in (True, False):
            ref, x, S = R.gemm_ref(A, W, bias if use_bias else None, epi, C0)
            outs = {}
            for kern in kernels if use_bias else [primary]:
                for pad in (PAD_COLS, 0) if (kern == primary and use_bias) else (PAD_COLS,):
                    C = guarded_launch(chk, shape, ops, epi, kern, use_bias, pad)
                    lab = (shape, "epi", epi, kern, use_bias, pad)
                    if epi >= 3:
                        chk.flag(lab, "f32 result != exact integer", (C.double() != ref).any())
                    elif epi == 0:
                        chk.flag(lab, "f16 result != RNE fp16 of the exact integer", (_bits(C) != _bits(ref.half())).any())
                    else:
                        chk.ratio((primary, "int", epi), lab, ((C.double() - ref).abs() / gemm_bound(ref, S, K, epi)).max())
                    outs[(kern, pad)] = C
            first = outs[(primary, PAD_COLS)]
            for key, C in outs.items():
                chk.flag((shape, "epi", epi, key, use_bias), "bytes differ from " + primary, (_bits(C) != _bits(first)).any())
            if epi == R.GEMM_RESIDUAL and use_bias:  # the accumulation happens once per launch
                C2 = guarded_launch(chk, (shape, "second residual launch"), ops, epi, primary, c_init=first)
                prod = ref - C0.double()
                chk.flag((shape, primary), "second residual launch != C0 + 2 * product",
                         (C2.double() != C0.double() + 2 * prod).any())


# ---- (a) exact cases ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [128, 384])
def test_k3_exact_tile_edges(cuda, N):
    """K3 forced on integer operands at every M around its 16 / 64 / 128-row blocks, grids of 1, 2, 3,
    6, 8, 9 and 24 workgroups (xcd_remap below, at and off a multiple of 8), one to three k-steps."""
    chk = _Checks()
    grids = set()
    for i, (M, n, K, _why) in enumerate(K3_SHAPES):
        if n != N:
            continue
        grids.add(-(-M // 128) * (n // 128))
        _exact_shape(chk, cuda, M, n, K, "k3", seed=100 + i)
    assert grids == ({1, 2, 3, 8} if N == 128 else {3, 6, 9, 24})
    worst = chk.finish()
    record_numerics(f"gemm_k3_exact_N{N}", [], [], **{f"epi{k[2]}_max_err_over_bound": v[0] for k, v in worst.items()})


@pytest.mark.parametrize("MB", [1, 2, 3, 4])
def test_k3s_exact_ring_edges(cuda, MB):
    """K3s (forced, and the automatic rule) at the edges of each MB class and with the k-pair count
    below, at, one and two past the ring depth RP, and past a second wrap; bytes equal to K3's."""
    chk = _Checks()
    n = 0
    for i, (M, N, K, _why) in enumerate(K3S_SHAPES):
        if (M + 15) // 16 != MB:
            continue
        n += 1
        _exact_shape(chk, cuda, M, N, K, "k3s", seed=300 + i)
    assert n == 7 * 3  # seven k-pair counts x three M (M = 1 is the first of MB = 1)
    worst = chk.finish()
    record_numerics(f"gemm_k3s_exact_MB{MB}", [], [], **{f"epi{k[2]}_max_err_over_bound": v[0] for k, v in worst.items()})


@pytest.mark.parametrize("K", [64, 128, 192])
def test_k3d_exact_block_edges(cuda, K):
    """K3d forced with one tile per workgroup and a stream of 4 (K = 64: the short-stream waits), 8 and
    12 half-tiles, M at every 16 / 64 / 128 / 256-row boundary of the ragged last tile (where the
    store count that feeds the next vmcnt changes); N = 512 and N = 4096 at K = 64."""
    chk = _Checks()
    for i, (M, N, k, _why) in enumerate(K3D_SHAPES):
        if k == K:
            _exact_shape(chk, cuda, M, N, k, "k3d", seed=500 + i)
    worst = chk.finish()
    record_numerics(f"gemm_k3d_exact_K{K}", [], [], **{f"epi{k[2]}_max_err_over_bound": v[0] for k, v in worst.items()})


@pytest.mark.parametrize("K", [64, 128])
def test_k3d_exact_persistent_loop(cuda, K):
    """K3d's persistent loop: N = 2304 (nine tile columns) and enough tile rows that every workgroup
    owns two or three tiles, the last row of tiles ragged (M = 256 rows - 100); epilogues 0 and 3."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    rows = -(-(2 * cus + 9) // 9)
    M, N = 256 * rows - 100, 2304
    nwg = max(8, cus // 8 * 8)
    ntiles = rows * 9
    assert 2 * nwg < ntiles <= 3 * nwg, (cus, ntiles)  # two and three tiles per workgroup
    chk = _Checks()
    _exact_shape(chk, cuda, M, N, K, "k3d", seed=700 + K, epis=(0, 3))
    chk.finish()


@pytest.mark.parametrize("N,K", [(256, 512), (384, 512), (256, 384), (384, 384), (2048, 512), (1536, 384)])
def test_k3w_exact_tiles(cuda, N, K):
    """K3w (forced, and the automatic rule) in its four <NB, KT> instantiations at M = 4096, 4097,
    4159, 4160 (the 64-row tile edges; with P = 1 or 2 panels most row ranges own one tile or none),
    and with three and four tiles per workgroup at M = 6500; bytes equal to K3's (and K3d's)."""
    chk = _Checks()
    n = 0
    for i, (M, n_, k, _why) in enumerate(K3W_SHAPES):
        if (n_, k) == (N, K):
            n += 1
            _exact_shape(chk, cuda, M, N, K, "k3w", seed=900 + i, epis=range(3))
    assert n >= 1
    chk.finish()


@pytest.mark.parametrize("M,N,K,R256", K3W_FLAT_MAP)
def test_k3w_exact_flat_block_map(cuda, M, N, K, R256):
    """K3w's xcd_map == 0 block map (p = b % P, r = b / P), which launch_ws takes when the row split
    R is below 8 or rounding it to the XCD count would idle more than 10 % of the CUs: the map a
    small partition takes everywhere. P and R as launch_ws computes them; the case asserts the map."""
    cus = max(8, torch.cuda.get_device_properties(cuda).multi_processor_count)
    nb4 = N % 256 == 0 and not (K == 384 and N % 192 == 0)  # launch_gemm_ws
    P = N // (64 * (4 if nb4 else 3))
    Rr = max(1, cus // P)
    xcd_map = Rr >= 8 and (Rr // 8 * 8) * 10 >= Rr * 9
    print("K3w flat map: cus", cus, "P", P, "R", Rr, "xcd_map", int(xcd_map))
    assert not xcd_map, ("this device would take the XCD map", cus, P, Rr)
    if cus == 256:
        assert Rr == R256
    chk = _Checks()
    _exact_shape(chk, cuda, M, N, K, "k3w", seed=1100 + K, epis=range(3))
    chk.finish()


@pytest.mark.parametrize("B,kernel,N", [(1, "auto", 384), (17, "auto", 384), (64, "auto", 384), (64, "k3s", 384),
                                        (65, "auto", 384), (300, "auto", 384), (300, "k3", 384),
                                        (1100, "k3d", 256), (1100, "auto", 256), (1100, "k3", 256)])
def test_strided_a_rows(cuda, B, kernel, N):
    """The cross-encoder pooler's operand: A = token 0 of each sequence of a [B][T][D] fp16 buffer
    (lda = T * D) whose other rows are NaN, epilogue 4: the bytes of the same rows packed densely.
    B <= 64 takes K3s, above K3; K3d (N % 256 == 0 only, so N = 256) forced and through the rule."""
    T, D = 5, 384
    A, W, bias, C0 = R.gemm_real_operands("plain", B, N, D, seed=B, device=cuda)
    buf = torch.full((B, T, D), float("nan"), dtype=torch.float16, device=cuda)
    buf[:, 0] = A
    chk = _Checks()
    dense = _Ops(A, W, bias, C0, cuda)
    strided = _Ops(A, W, bias, C0, cuda)
    strided.abuf, strided.A, strided.lda = buf, buf.view(B * T, D)[::T], T * D
    strided.keep = (buf.clone(),) + strided.keep[1:]
    ref, x, S = R.gemm_ref(A, W, bias, 4)
    cd = guarded_launch(chk, (B, "dense"), dense, 4, kernel)
    cs = guarded_launch(chk, (B, "strided"), strided, 4, kernel)
    chk.flag((B, kernel), "strided A != dense A bytes", (_bits(cd) != _bits(cs)).any())
    chk.ratio(("strided", kernel), B, ((cs.double() - ref).abs() / gemm_bound(ref, S, D, 4)).max())
    chk.finish()


# ---- (b) real operands against float64, per element ----------------------------------------------
# (kernel, M, N, K): one shape per kernel from the lists above, K3 / K3d at K = 768, K3w at both K.
# Observed max err / bound on MI355X is printed per (kernel, epilogue) and recorded (numerics section).
REAL_SHAPES = [
    ("k3", 257, 384, 192), ("k3", 1000, 384, 768),
    ("k3s", 33, 128, 704), ("k3s", 64, 128, 448),
    ("k3d", 1153, 256, 192), ("k3d", 1100, 512, 768),
    ("k3w", 4159, 384, 384), ("k3w", 4097, 256, 512),
]


@pytest.mark.parametrize("kernel", ["k3", "k3s", "k3d", "k3w"])
def test_gemm_real_operands_against_float64(cuda, kernel):
    """(b): every kernel on plain and cancelling operands, every epilogue it has, each element
    within the derived bound of the module docstring of the float64 result; bytes equal to K3's."""
    chk = _Checks()
    for kern, M, N, K in REAL_SHAPES:
        if kern != kernel:
            continue
        for kind in R.GEMM_KINDS:
            A, W, bias, C0 = R.gemm_real_operands(kind, M, N, K, seed=M + K, device=cuda)
            ops = _Ops(A, W, bias, C0, cuda)
            for epi in range(3 if kernel == "k3w" else 5):
                ref, x, S = R.gemm_ref(A, W, bias, epi, C0)
                lab = ((M, N, K), kind)
                C = guarded_launch(chk, lab, ops, epi, kernel)
                chk.ratio((kernel, epi), lab, ((C.double() - ref).abs() / gemm_bound(ref, S, K, epi)).max())
                if kind == "cancel" and epi in (3, 4):  # the same with the rounding's own scale only
                    chk.ratio((kernel, epi, "cancel / ACC"), lab, ((C.double() - ref).abs() / R.gemm_acc_bound(S, K)).max())
                if kernel != "k3":
                    C3 = guarded_launch(chk, lab, ops, epi, "k3")
                    chk.flag((lab, epi), "bytes differ from K3", (_bits(C) != _bits(C3)).any())
    worst = chk.finish()
    for epi in range(3 if kernel == "k3w" else 5):
        record_numerics(f"gemm_{kernel}_epi{epi}_vs_float64", [], [], max_err_over_bound=worst[(kernel, epi)][0],
                        worst_case=str(worst[(kernel, epi)][1]))


# ---- (c) quick-GELU sweep --------------------------------------------------------------------------
def test_quick_gelu_epilogue_sweep(cuda):
    """The quick-GELU epilogue (hardware exp2 / rcp) swept over x in [-16, 16) in steps of 2^-14
    (x = A[r, 0] * W[n, 0] + bias[n] = (r / 4 - 16) + n / 16384, exact in f32, one launch), and rows
    at |x| = 30, 100, 1000 where exp2 under- and overflows: -0 / x there, never NaN; against float64
    x sigmoid(1.702 x) within fp16 rounding + the absolute term of the module docstring."""
    M0, N, K = 128, 4096, 64
    far = [30.0, -30.0, 100.0, -100.0, 1000.0, -1000.0]
    M = M0 + len(far)
    A = torch.zeros(M, K, dtype=torch.float16)
    A[:M0, 0] = torch.arange(M0, dtype=torch.float32) / 4 - 16
    A[M0:, 0] = torch.tensor(far)
    W = torch.zeros(N, K, dtype=torch.float16)
    W[:, 0] = 1.0
    bias = torch.arange(N, dtype=torch.float32) / 16384
    chk = _Checks()
    ops = _Ops(A.to(cuda), W, bias, None, cuda)
    out = guarded_launch(chk, "sweep", ops, R.GEMM_QUICK_GELU, "auto")
    x = ops.A[:, :1].double() + ops.bias.double()[None, :]
    assert torch.equal(x.float().double(), x)  # exact in f32
    ref = R.gemm_act_ref(x, R.GEMM_QUICK_GELU)
    err = (out.double() - ref).abs()
    bound = F16_EPS * ref.abs() + 2.0 ** -25 + QGELU_ABS + ACT_REL * ref.abs()
    chk.ratio("quick_gelu_sweep", "all rows", (err / bound).max())
    big_pos = (x >= 100).expand_as(out)
    big_neg = (x <= -100).expand_as(out)
    chk.flag("sweep", "x >= 100 does not give fp16(x)", (out[big_pos] != x.expand_as(out)[big_pos].half()).any())
    chk.flag("sweep", "x <= -100 does not give zero", (out[big_neg] != 0).any())
    worst = chk.finish()
    excess = (err - F16_EPS * ref.abs() - 2.0 ** -25).max()
    record_numerics("quick_gelu_epilogue_sweep", out[:M0].float().cpu().numpy()[52:], ref[:M0].float().cpu().numpy()[52:],
                    unit=False, max_err_over_bound=worst["quick_gelu_sweep"][0], max_abs_err=float(err.max()),
                    max_err_beyond_fp16_rounding=float(excess), neg_zero_rows_signbit=bool(torch.signbit(out[big_neg].float()).all()))


# ---- (d) fp16 subnormal operands -------------------------------------------------------------------
@pytest.mark.parametrize("kernel,M,N,K", [("k3", 129, 128, 192), ("k3s", 17, 128, 704)])
def test_gemm_fp16_subnormal_operands(cuda, kernel, M, N, K):
    """A = integers in [-4, 4] times 2^-24 (fp16 subnormals, which LayerNorm's f16 copy produces), W
    integers, epilogue 4: every product and partial sum is a multiple of 2^-24 below 2^-8, exact in
    f32, provided the f16 MFMA does not flush subnormal inputs. It does not (observed on MI355X, K3 and
    K3s: the exact product; DESIGN.md, GEMM numerics), so the exact product is asserted."""
    Ai, W, bias, _ = R.gemm_int_operands(M, N, K, seed=K, device=cuda)
    A = (Ai.double() * 2.0 ** -24).half()
    assert bool((A.double() == Ai.double() * 2.0 ** -24).all())
    bias = bias * 2.0 ** -24
    chk = _Checks()
    ops = _Ops(A, W, bias, None, cuda)
    ref, x, S = R.gemm_ref(A, W, bias, 4)
    C = guarded_launch(chk, "subnormal", ops, 4, kernel)
    C3 = guarded_launch(chk, "subnormal", ops, 4, "k3")
    chk.flag("subnormal", "kernels differ in bytes", (_bits(C) != _bits(C3)).any())
    chk.flag("subnormal", "not the exact product (subnormal inputs flushed?)", (C.double() != ref).any())
    worst = float(((C.double() - ref).abs() / S).max())
    print("fp16 subnormal A through the f16 MFMA: max |C - ref| / S = %.3g" % worst)
    record_numerics(f"gemm_{kernel}_fp16_subnormal_A", [], [], max_err_over_S=worst)
    chk.finish()


# ---- (e) the K3d offset guard on real buffers ----------------------------------------------------------
def test_k3d_offset_guard_large_batch(cuda):
    """(M - 1) * lda + K > INT_MAX with really allocated operands (699,256 x 3072 fp16, 4.3 GB): K3d
    forced is rejected before any launch (C keeps its pre-fill), the automatic rule runs K3 (size_t
    offsets): every row written, the first and last 300 rows within the bound of (b) and bit-identical
    to K3 on those rows alone."""
    from app import _native
    from app.encoders import gemm_nt

    M, N, K = 699_256, 256, 3072
    assert (M - 1) * K + K > 2 ** 31 - 1
    g = torch.Generator(device=cuda).manual_seed(9)
    A = torch.randn((M, K), dtype=torch.float16, device=cuda, generator=g)
    W = (torch.randn((N, K), device=cuda, generator=g) * 0.05).half()
    bias = torch.randn(N, device=cuda, generator=g) * 0.1
    cbuf = torch.empty((M + GUARD_ROWS, N), dtype=torch.float16, device=cuda)
    cbuf.view(torch.uint8).fill_(GUARD_BYTE)
    C = cbuf[:M]
    C[:] = float("nan")
    with pytest.raises(_native.NativeError, match="offset"):
        gemm_nt(A, W, bias, C, 0, kernel="k3d")
    assert bool(torch.isnan(C).all()), "rejected launch wrote C"
    gemm_nt(A, W, bias, C, 0)
    chk = _Checks()
    chk.flag("large", "NaN left in C", torch.isnan(C).any())
    chk.flag("large", "guard rows written", (_bits(cbuf[M:]) != _GUARD_WORD[2]).any())
    for name, rows in (("first", slice(0, 300)), ("last", slice(M - 300, M))):
        ref, x, S = R.gemm_ref(A[rows], W, bias, 0)
        chk.ratio(("large", name), name, ((C[rows].double() - ref).abs() / gemm_bound(ref, S, K, 0)).max())
        Cs = guarded_launch(chk, ("large", name, "alone"), _Ops(A[rows], W, bias, None, cuda), 0, "k3")
        chk.flag(("large", name), "rows differ from K3 on the rows alone", (_bits(Cs) != _bits(C[rows])).any())
    worst = chk.finish()
    record_numerics("gemm_auto_past_int32_offsets", [], [], max_err_over_bound=max(v[0] for v in worst.values()))
    del A, C, cbuf
    torch.cuda.empty_cache()
