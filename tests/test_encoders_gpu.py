"""Parity of the HIP encoders (libmrag.so via the C ABI) with the golden fixtures
produced by the reference's own code (oracle/gen_golden.py).

Tolerance (north_star: "cosine scores within 1e-4 fp32"): the GPU path computes in fp16
MFMA with f32 accumulation and an f32 residual stream; the reference runs fp32. Unit-norm
outputs must agree row by row to 1 - cos <= 1e-4 and max |diff| <= ABS_MAX per component;
the unnormalised features to REL_L2 relative L2 error. Every comparison's observed
errors are recorded (conftest.record_numerics) and printed at the end of the run. The K3
GEMM is checked against a torch fp32 product of the same fp16 inputs to 1e-2 relative.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from conftest import GOLDEN, record_numerics

pytestmark = pytest.mark.gpu

# Observed on MI355X (profiles/r2_numerics.json): 1 - cos <= 6e-7, |diff| <= 2.3e-4 on unit
# rows, relative L2 <= 1.1e-3 on unnormalised features, over every tower and BASELINE config.
COS_ERR_MAX = 1e-4   # 1 - cos(gpu row, oracle row), north_star
ABS_MAX = 1e-3       # per component of a unit row (typical component ~0.044 at 512-d)
REL_L2 = 5e-3        # unnormalised features


def _cmp(got, exp, unit=True, name="encoder"):
    row = record_numerics(name, got, exp, unit=unit)
    if unit:
        assert row["max_1_minus_cos"] <= COS_ERR_MAX, row
        assert row["max_abs_diff"] <= ABS_MAX, row
    else:
        assert row["max_rel_l2"] <= REL_L2, row


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
def test_gemm_epilogues(cuda, epi):
    import torch

    from app.encoders import gemm_nt

    g = torch.Generator(device=cuda).manual_seed(epi)
    M, N, K = 300, 384, 320
    A = (torch.randn(M, K, generator=g, device=cuda) * 0.5).half()
    W = (torch.randn(N, K, generator=g, device=cuda) * 0.05).half()
    bias = torch.randn(N, generator=g, device=cuda) * 0.1
    ref = A.float() @ W.float().t() + bias
    if epi == 1:
        ref = ref * torch.sigmoid(1.702 * ref)
    elif epi == 2:
        ref = torch.nn.functional.gelu(ref)
    if epi <= 2:
        C = torch.empty(M, N, dtype=torch.float16, device=cuda)
    elif epi == 3:
        C0 = torch.randn(M, N, generator=g, device=cuda)
        C = C0.clone()
        ref = ref + C0
    else:
        C = torch.empty(M, N, dtype=torch.float32, device=cuda)
    gemm_nt(A, W, bias, C, epi)
    torch.cuda.synchronize()
    err = (C.float() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-2, err


@pytest.mark.parametrize("M,N,K", [(1100, 768, 768), (2048, 384, 320), (1024, 2304, 192), (8300, 2304, 128),
                                   (2100, 1536, 256), (12800, 768, 3072)])
@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
def test_gemm_big_tiles(cuda, M, N, K, epi):
    """K3d (persistent 256 x 256 tiles, from M = 1024 when N % 256 == 0 and the 256 x 256 grid
    fills the CUs at least as well as K3 would; K3 otherwise):
    ragged M (1100 = 4 x 256 + 76, 8300), 297 tiles (> one per CU: the load stream and the
    epilogue stores run across tiles), every epilogue; same tolerance as K3."""
    import torch

    from app.encoders import gemm_nt

    g = torch.Generator(device=cuda).manual_seed(7 + epi)
    A = (torch.randn(M, K, generator=g, device=cuda) * 0.5).half()
    W = (torch.randn(N, K, generator=g, device=cuda) * 0.05).half()
    bias = torch.randn(N, generator=g, device=cuda) * 0.1
    ref = A.float() @ W.float().t() + bias
    if epi == 1:
        ref = ref * torch.sigmoid(1.702 * ref)
    elif epi == 2:
        ref = torch.nn.functional.gelu(ref)
    if epi <= 2:
        C = torch.full((M, N), float("nan"), dtype=torch.float16, device=cuda)
    elif epi == 3:
        C0 = torch.randn(M, N, generator=g, device=cuda)
        C = C0.clone()
        ref = ref + C0
    else:
        C = torch.full((M, N), float("nan"), dtype=torch.float32, device=cuda)
    gemm_nt(A, W, bias, C, epi)
    torch.cuda.synchronize()
    assert not torch.isnan(C.float()).any()
    err = (C.float() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-2, err


@pytest.fixture(scope="module")
def vision(cuda):
    from app.encoders import CLIP_VISION_B32, GpuEncoder

    return GpuEncoder(CLIP_VISION_B32)


def test_clip_image_golden(vision):
    g = np.load(os.path.join(GOLDEN, "golden_clip_image.npz"))
    _cmp(vision.embed_images(g["images_u8"]), g["expected"], name="clip_image_golden")
    _cmp(vision.embed_images(g["images_u8"], normalize=False), g["expected_unnormalized"], unit=False,
         name="clip_image_golden_unnormalized")


def test_clip_image_device_batch_consistency(vision, cuda):
    """Batch size must not change a row's result (padding rows / tiling), bit for bit: every
    hand-written GEMM kernel (K3 under 1024 rows, K3d above) accumulates an element in one order
    and finishes it with one epilogue, and LayerNorm / attention rows are independent."""
    import torch

    g = np.load(os.path.join(GOLDEN, "golden_clip_image.npz"))
    imgs = np.concatenate([g["images_u8"]] * 50)[:131]  # ragged batch, > one 128-row tile
    b = vision.embed_images(imgs[:3])
    small = vision.embed_images(torch.from_numpy(imgs[:61]).to(cuda)).cpu().numpy()  # 3050 rows
    np.testing.assert_array_equal(small[:3], b)
    np.testing.assert_array_equal(small[3:6], b)
    a = vision.embed_images(torch.from_numpy(imgs).to(cuda)).cpu().numpy()  # 6550 rows
    for blk in (a[:3], a[3:6], a[126:129]):
        np.testing.assert_array_equal(blk, b)


def test_batches_in_flight_bit_identical(vision, cuda):
    """The bench's work-in-flight form (bench_clip_images): three encoder handles, each batch on
    its own stream, enqueued from one thread without host syncs; every batch's embeddings equal
    the serial call's bit for bit (same weights, independent workspaces). Batches of 40-160
    images (K3 and K3d GEMMs)."""
    import torch

    from app.encoders import CLIP_VISION_B32, GpuEncoder

    g = torch.Generator(device=cuda).manual_seed(9)
    batches = [torch.randint(0, 256, (40 + 24 * i, 224, 224, 3), generator=g, dtype=torch.uint8, device=cuda)
               for i in range(6)]
    serial = [vision.embed_images(b).cpu() for b in batches]
    encs = [GpuEncoder(CLIP_VISION_B32) for _ in range(3)]
    streams = [torch.cuda.Stream(device=cuda) for _ in range(3)]
    outs = [None] * len(batches)
    for i, b in enumerate(batches):
        with torch.cuda.stream(streams[i % 3]):
            outs[i] = encs[i % 3].embed_images(b)
    torch.cuda.synchronize()
    for i in range(len(batches)):
        assert torch.equal(outs[i].cpu(), serial[i]), i


def test_clip_text_golden(cuda):
    from app.encoders import CLIP_TEXT_B32, GpuEncoder

    g = np.load(os.path.join(GOLDEN, "golden_clip_text.npz"))
    enc = GpuEncoder(CLIP_TEXT_B32)
    _cmp(enc.embed_tokens(g["ids"], g["mask"]), g["expected"], name="clip_text_golden")
    _cmp(enc.embed_tokens(g["ids"], g["mask"], normalize=False), g["expected_unnormalized"], unit=False,
         name="clip_text_golden_unnormalized")


def test_minilm_golden(cuda):
    from app.encoders import MINILM_L6, GpuEncoder

    g = np.load(os.path.join(GOLDEN, "golden_minilm.npz"))
    enc = GpuEncoder(MINILM_L6)
    _cmp(enc.embed_tokens(g["ids"], g["mask"]), g["expected"], name="minilm_golden")
    _cmp(enc.embed_tokens(g["ids"], g["mask"], normalize=False), g["expected_unnormalized"], unit=False,
         name="minilm_golden_unnormalized")


def test_minilm_max_length_256(cuda):
    """ST max_seq_length 256: the longest sequence the reference feeds MiniLM."""
    from app.encoders import MINILM_L6, GpuEncoder
    from oracle.models import bert_model, minilm_embeds

    rng = np.random.default_rng(5)
    ids = rng.integers(1000, 30000, (3, 256)).astype(np.int32)
    ids[:, 0], ids[:, -1] = 101, 102
    mask = np.ones_like(ids)
    mask[1, 200:] = 0
    enc = GpuEncoder(MINILM_L6)
    _cmp(enc.embed_tokens(ids, mask), minilm_embeds(bert_model(0), ids, mask), name="minilm_L256")


def test_gemm_shapes_every_epilogue(cuda):
    """K3 / K3d against a torch fp32 product of the same fp16 operands, every epilogue, on ragged
    M and the encoders' N / K (K3d for M >= 1024 where its grid wins, K3 otherwise); repeated
    launches bit-identical."""
    import torch
    from app.encoders import gemm_nt

    for (M, N, K) in [(1100, 768, 768), (2100, 1536, 256), (12800, 768, 3072), (12800, 2304, 768),
                      (300, 256, 64), (5000, 512, 2048), (16000, 384, 1536), (12800, 768, 768),
                      (12800, 3072, 768), (11000, 768, 3072)]:
        for epi in range(5):
            g = torch.Generator(device="cuda").manual_seed(epi + K)
            A = (torch.randn(M, K, generator=g, device="cuda") * 0.5).half()
            W = (torch.randn(N, K, generator=g, device="cuda") * 0.05).half()
            bias = torch.randn(N, generator=g, device="cuda") * 0.1
            ref = A.float() @ W.float().t() + bias
            if epi == 1:
                ref = ref * torch.sigmoid(1.702 * ref)
            elif epi == 2:
                ref = torch.nn.functional.gelu(ref)
            C0 = torch.randn(M, N, generator=g, device="cuda") if epi == 3 else None
            outs = []
            for _ in range(2):
                if epi <= 2:
                    C = torch.full((M, N), float("nan"), dtype=torch.float16, device="cuda")
                elif epi == 3:
                    C = C0.clone()
                else:
                    C = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
                gemm_nt(A, W, bias, C, epi)
                torch.cuda.synchronize()
                outs.append(C)
            r = ref + C0 if epi == 3 else ref
            C = outs[0]
            assert not torch.isnan(C.float()).any(), (M, N, K, epi)
            assert torch.equal(outs[0], outs[1]), ("nondeterministic", M, N, K, epi)
            err = (C.float() - r).abs().max().item() / r.abs().max().item()
            assert err < (2e-3 if epi <= 2 else 2e-5), (M, N, K, epi, err)
    # bias == NULL (the ViT patch embedding and both CLIP projections): K3 and K3d forced, an f16 and an f32 epilogue, against A W^T
    for kern, (M, N, K) in (("k3", (300, 256, 64)), ("k3d", (1100, 768, 768))):
        g = torch.Generator(device="cuda").manual_seed(K)
        A = (torch.randn(M, K, generator=g, device="cuda") * 0.5).half()
        W = (torch.randn(N, K, generator=g, device="cuda") * 0.05).half()
        ref = A.float() @ W.float().t()
        for epi in (0, 4):
            C = torch.full((M, N), float("nan"), dtype=torch.float16 if epi == 0 else torch.float32, device="cuda")
            gemm_nt(A, W, None, C, epi, kernel=kern)
            torch.cuda.synchronize()
            assert not torch.isnan(C.float()).any(), (kern, epi)
            err = (C.float() - ref).abs().max().item() / ref.abs().max().item()
            assert err < (2e-3 if epi == 0 else 2e-5), (kern, "bias=None", epi, err)


@pytest.mark.parametrize("N,K", [(384, 384), (384, 1536), (1152, 384), (1536, 384), (512, 2048), (2048, 512),
                                 (768, 3072), (2304, 768), (128, 64), (256, 128)])
def test_gemm_skinny_rows_equal_k3(cuda, N, K):
    """K3s (M <= 64: one query / one image per call) against K3 on the same rows: every epilogue,
    M = 1, 5, 16, 17, 33, 50, 64 (1-4 activation blocks, ragged), bit-identical to rows 0..M-1 of
    a 200-row K3 call over the same A rows (so a query's embedding does not depend on its batch
    size), and within the K3 tolerance of a torch fp32 product; K from 64 (one k-pair, no ring
    wrap) to 3072 (the ring wraps several times)."""
    import torch

    from app.encoders import gemm_nt

    g = torch.Generator(device=cuda).manual_seed(N + K)
    Mb = 200
    A = (torch.randn(Mb, K, generator=g, device=cuda) * 0.5).half()
    W = (torch.randn(N, K, generator=g, device=cuda) * 0.05).half()
    bias = torch.randn(N, generator=g, device=cuda) * 0.1
    C0 = torch.randn(Mb, N, generator=g, device=cuda)
    for epi in range(5):
        def run(M):
            if epi <= 2:
                C = torch.full((M, N), float("nan"), dtype=torch.float16, device=cuda)
            elif epi == 3:
                C = C0[:M].clone()
            else:
                C = torch.full((M, N), float("nan"), dtype=torch.float32, device=cuda)
            gemm_nt(A[:M].contiguous(), W, bias, C, epi)
            return C

        big = run(Mb)
        ref = A.float() @ W.float().t() + bias
        if epi == 1:
            ref = ref * torch.sigmoid(1.702 * ref)
        elif epi == 2:
            ref = torch.nn.functional.gelu(ref)
        if epi == 3:
            ref = ref + C0
        for M in (1, 5, 16, 17, 33, 50, 64):
            C = run(M)
            torch.cuda.synchronize()
            assert not torch.isnan(C.float()).any(), (M, epi)
            assert torch.equal(C, big[:M]), ("skinny != K3 rows", M, N, K, epi)
            err = (C.float() - ref[:M]).abs().max().item() / ref[:M].abs().max().item()
            assert err < (2e-3 if epi <= 2 else 2e-5), (M, N, K, epi, err)
    if (N, K) == (384, 384):  # bias == NULL on K3s: the same bytes as K3's rows, and A W^T
        ref = A.float() @ W.float().t()
        outs = {}
        for kern, M in (("k3", Mb), ("k3s", 17)):
            C = torch.full((M, N), float("nan"), dtype=torch.float16, device=cuda)
            gemm_nt(A[:M].contiguous(), W, None, C, 0, kernel=kern)
            outs[kern] = C
        torch.cuda.synchronize()
        assert not torch.isnan(outs["k3s"].float()).any()
        assert torch.equal(outs["k3s"], outs["k3"][:17]), "skinny != K3 rows, bias=None"
        err = (outs["k3s"].float() - ref[:17]).abs().max().item() / ref[:17].abs().max().item()
        assert err < 2e-3, ("bias=None", err)


@pytest.mark.parametrize("N,K", [(1536, 512), (2048, 512), (1152, 384), (1536, 384), (768, 512), (384, 384),
                                 (1152, 512), (384, 512)])
def test_gemm_weight_stationary_equals_k3(cuda, N, K):
    """K3w (the weight-stationary kernel the text towers' q|k|v and fc1 take at K 384 / 512) against
    K3 forced on the same operands: bit-identical for the three f16 epilogues (one accumulation
    order, K3's epilogue), with M a multiple of the 64-row tile, ragged (the last tile partly past
    M: clamped loads, no stores), and small enough that some row ranges own no tile or one tile;
    and within K3's tolerance of a torch fp32 product. The automatic rule takes K3w for these
    shapes at M >= 4096. (1152, 512) and (384, 512) are K = 512 with N % 192 == 0 only: three
    64-column blocks per wave at the 16-step K. Without a bias (as the CLIP projections call it): the same
    checks at one K = 384 and one K = 512 shape."""
    import torch

    from app.encoders import gemm_nt

    g = torch.Generator(device=cuda).manual_seed(7 * N + K)
    for M in (16000, 4100, 4096 + 63, 5000):
        A = (torch.randn(M, K, generator=g, device=cuda) * 0.5).half()
        W = (torch.randn(N, K, generator=g, device=cuda) * 0.05).half()
        bias = torch.randn(N, generator=g, device=cuda) * 0.1
        ref = A.float() @ W.float().t() + bias
        for epi in range(3):
            outs = {}
            for kern in ("k3", "k3w", "auto"):
                C = torch.full((M, N), float("nan"), dtype=torch.float16, device=cuda)
                gemm_nt(A, W, bias, C, epi, kernel=kern)
                outs[kern] = C
            torch.cuda.synchronize()
            assert not torch.isnan(outs["k3w"].float()).any(), (M, N, K, epi)
            assert torch.equal(outs["k3w"], outs["k3"]), ("K3w != K3", M, N, K, epi)
            assert torch.equal(outs["auto"], outs["k3"]), ("auto != K3", M, N, K, epi)  # whichever kernel auto picks
            if epi == 0:
                err = (outs["k3w"].float() - ref).abs().max().item() / ref.abs().max().item()
                assert err < 2e-3, (M, N, K, err)
        if M == 4100 and (N, K) in ((1152, 384), (384, 512)):
            ref0 = A.float() @ W.float().t()
            for epi in range(3):
                outs = {}
                for kern in ("k3", "k3w"):
                    C = torch.full((M, N), float("nan"), dtype=torch.float16, device=cuda)
                    gemm_nt(A, W, None, C, epi, kernel=kern)
                    outs[kern] = C
                torch.cuda.synchronize()
                assert not torch.isnan(outs["k3w"].float()).any(), ("bias=None", N, K, epi)
                assert torch.equal(outs["k3w"], outs["k3"]), ("K3w != K3, bias=None", N, K, epi)
                if epi == 0:
                    err = (outs["k3w"].float() - ref0).abs().max().item() / ref0.abs().max().item()
                    assert err < 2e-3, ("bias=None", N, K, err)


def test_gelu_erf_epilogue_sweep(cuda):
    """the erf-GELU epilogue (A&S 7.1.26 + hardware rcp/exp2) swept over x in
    [-8, 8) against torch.nn.functional.gelu (exact erf) on the fp16 output, with an absolute
    bound: fp16 rounding of the result (half an ulp, <= 2^-11 relative) + 2e-6 absolute.
    x = A[r,0] * W[n,0] + bias[n] = (r/8 - 8) + n/32768, exact in f32 (one launch)."""
    import torch

    from app.encoders import gemm_nt

    M, N, K = 128, 4096, 64
    A = torch.zeros(M, K, dtype=torch.float16, device=cuda)
    A[:, 0] = torch.arange(M, device=cuda, dtype=torch.float32) / 8 - 8
    W = torch.zeros(N, K, dtype=torch.float16, device=cuda)
    W[:, 0] = 1.0
    bias = torch.arange(N, device=cuda, dtype=torch.float32) / 32768
    out = torch.empty(M, N, dtype=torch.float16, device=cuda)
    gemm_nt(A, W, bias, out, 2)  # epilogue 2 = gelu_erf(acc + bias)
    torch.cuda.synchronize()
    x = A[:, :1].double() + bias.double()[None, :]
    ref = torch.nn.functional.gelu(x)
    err = (out.double() - ref).abs()
    bound = ref.abs() * 2.0 ** -11 + 2e-6
    assert bool((err <= bound).all()), float((err - bound).max())
    neg = x < -3.5
    # the recorded rows: x in [-3.5, 8), where the output is not ~0, so the cosine and the relative
    # L2 of each 4096-wide row mean something (the rows below -3.5 are covered by the absolute bound)
    keep = slice(36, M)  # r / 8 - 8 >= -3.5
    record_numerics("gelu_erf_epilogue_sweep", out.float().cpu().numpy()[keep], ref.float().cpu().numpy()[keep],
                    unit=False, max_abs_err=float(err.max()), max_abs_err_x_below_m3p5=float(err[neg].max()))


@pytest.mark.parametrize("tower", ["minilm", "clip_text"])
def test_padding_invariance(cuda, tower):
    """A sequence's embedding does not depend on how far its batch is padded (K4 v3 skips fully
    masked key blocks; every other block, GEMM row, LayerNorm row and the pooling are
    per-sequence): each sequence alone == the same sequence inside a batch padded to the
    longest, bit for bit, for lengths across the 16-key block boundaries and past 64."""
    from app.encoders import CLIP_TEXT_B32, MINILM_L6, GpuEncoder

    cfg = MINILM_L6 if tower == "minilm" else CLIP_TEXT_B32
    lens = [3, 16, 17, 40, 64, 65, 77] + ([130, 256] if tower == "minilm" else [])
    T = max(lens)
    rng = np.random.default_rng(17)
    ids = np.zeros((len(lens), T), np.int32)
    mask = np.zeros((len(lens), T), np.int32)
    for i, n in enumerate(lens):
        if tower == "minilm":
            ids[i, :n] = rng.integers(1000, 30000, n)
            ids[i, 0], ids[i, n - 1] = 101, 102
        else:
            ids[i, :n] = rng.integers(1, 49405, n)
            ids[i, 0], ids[i, n - 1] = 49406, 49407
            ids[i, n:] = 49407  # CLIP pads with the EOS id (first EOS pooling)
        mask[i, :n] = 1
    enc = GpuEncoder(cfg)
    batch = enc.embed_tokens(ids, mask)
    for i, n in enumerate(lens):
        alone = enc.embed_tokens(ids[i:i + 1, :n], mask[i:i + 1, :n])
        np.testing.assert_array_equal(alone[0], batch[i], err_msg=f"length {n}")


@pytest.mark.parametrize("tower", ["minilm", "clip_text"])
def test_small_batch_graph_replay_bit_identical(cuda, tower):
    """Host-pointer calls of up to 2048 tokens replay a captured hipGraph of the forward (the
    reference's one-query-per-retrieve pattern); device-pointer calls launch directly. Same
    kernels in the same order: bit-identical, across replays with new ids, alternating lengths
    (one graph per shape) and a workspace that grows between replays (its buffers move: the
    graph must be recaptured, not replayed against freed memory)."""
    import torch

    from app.encoders import CLIP_TEXT_B32, MINILM_L6, GpuEncoder

    cfg = MINILM_L6 if tower == "minilm" else CLIP_TEXT_B32
    enc = GpuEncoder(cfg)
    rng = np.random.default_rng(23)

    def query(b, n):
        if tower == "minilm":
            ids = rng.integers(1000, 30000, (b, n)).astype(np.int32)
            ids[:, 0], ids[:, -1] = 101, 102
        else:
            ids = rng.integers(1, 49405, (b, n)).astype(np.int32)
            ids[:, 0], ids[:, -1] = 49406, 49407
        return ids, np.ones_like(ids)

    def both(ids, mask):
        host = enc.embed_tokens(ids, mask)
        dev = enc.embed_tokens(torch.from_numpy(ids).to(cuda), torch.from_numpy(mask).to(cuda))
        torch.cuda.synchronize()
        return host, dev.cpu().numpy()

    for b, n in [(1, 5), (1, 12), (1, 5), (4, 9), (1, 12), (1, 5)]:
        h, d = both(*query(b, n))
        np.testing.assert_array_equal(h, d, err_msg=f"B={b} T={n}")
    big = query(64, 40)  # 2560 tokens: direct launches, and the workspace grows
    h, d = both(*big)
    np.testing.assert_array_equal(h, d)
    for b, n in [(1, 5), (1, 12)]:  # the old graphs baked the freed buffers: recaptured
        h, d = both(*query(b, n))
        np.testing.assert_array_equal(h, d, err_msg=f"after growth B={b} T={n}")


def test_workspace_per_sequence_buffers_grow_alone(cuda):
    """The workspace's per-sequence buffers grow with B, its per-token ones with B * T: after
    (B, T) = (2, 16), a batch of (4, 8) has as many tokens and twice the sequences, so only the
    per-sequence buffers are made again. Each result on the one handle == the same batch on a
    fresh handle, bit for bit."""
    from app.encoders import MINILM_L6, GpuEncoder

    rng = np.random.default_rng(29)
    enc = GpuEncoder(MINILM_L6)
    for b, n in [(2, 16), (4, 8)]:
        ids = rng.integers(1000, 30000, (b, n)).astype(np.int32)
        ids[:, 0], ids[:, -1] = 101, 102
        mask = np.ones_like(ids)
        got = enc.embed_tokens(ids, mask)
        np.testing.assert_array_equal(got, GpuEncoder(MINILM_L6).embed_tokens(ids, mask), err_msg=f"B={b} T={n}")
