"""AVL_OP_GEMM alone, on operands whose every product is exactly computable: bit equality on everything the op writes.

Why.  The "mixed" GEMMs add correction products (W lo . x hi, W hi . x lo) to the f16 main product.  On Gaussian operands a
correction pass is ~1e-4 of max|ref|, far inside the 2^-11 * 1.5 a single f16 output plane is allowed in test_gpu_mixed.py: a
kernel that drops a pass, reads the wrong weight block or ignores a residual's lo plane passes there.  Here every term is as
large as the main product and the result is known to the bit.

Operand design.
  * Small values.  Every matrix element is one of {0, +-1, +-2, +-3, +-4, +-6} (the e2m1 grid's integers), zeros frequent, some
    32-blocks all zero or holding one non-zero.  The two FP4 halves of an activation bundle are in addition scaled per row by
    2^-1, 1 or 2.  Such values pass through mx_quant_fp4 / mx_dequant_fp4 unchanged (asserted when the operands are built), f16
    holds them exactly, and every product and partial sum is a multiple of 1/2 of magnitude at most 3 * K * 6 * 6 * 2 = 216 K
    <= 2^19 for K <= 2048 -- 2^20 halves, under 2^24, so fp32 accumulation is exact in ANY order and the fp32 matrix product on
    the host is the float64 one.
  * Decoupled.  The ABI defines the MX products on what the caller passes, so each operand comes from a matrix of its own:
        in = A (f16 plane), in_mx = [Q4(B) | Q4(C)], weight = Wh (f16 rows), w_mx = [Q4(Wl) | Q4(Wh')]
        accumulator = A . Wh^T + B . Wl^T [+ C . Wh'^T] + bias          (third term: in_lo set or AVL_MX_IN_LO)
    The three terms are of one size, so a dropped, doubled or mis-paired pass moves most outputs by hundreds of ulps.  in_lo is a
    NaN-filled plane: the MX GEMM reads the lo operand from the bundle, in_lo only switches the pass on (include/avl_hip.h).
    A second input (in3 / in3_mx) is three more independent matrices over the appended K range.
  * Split GEMM (w_split = 1): weight = [n][K/64][W1 64 | W2 64 (| W3 64)] assembled by hand from independent matrices,
        accumulator = A . W1^T + A . W2^T [+ A_lo . W3^T] + bias
    W3 differs from W1, so a pass that multiplies the lo plane with the wrong block shows.
  * Bias: integers, a quarter of the columns beyond +-2048 (the hi plane then rounds and the lo part is non-zero).  Residual:
    an integer f16 plane + nothing | an integer f16 lo plane | an FP4 lo half of in2_mx whose hi half is random bytes.
  * Sums are negative about half the time; cases alternate ReLU on / off.

Expected, with v the exact result: out = f16(v) (round to nearest even), out_lo = f16(v - out), Q4(hi) half of out_mx =
mx_quant_fp4(out) byte for byte with its scales, lo half = mx_quant_fp4 of the f16 lo plane when out_lo is set and of the
fp32 value v - out under AVL_MX_OUT_LO alone.  Rows past M keep their sentinel in every plane and scale slab; so do out_lo and
the lo half of the bundle when the form does not write them.

Which kernel a case reaches is part of the case (the last field of MX_CASES, SPLIT_KERNELS) and asserted against the library's own
answer for the very op that runs (avl_seg_gemm_route, whose comment in include/avl_hip.h states the rule; t256 there = ceil(M / 256)
* N / 256 on ONE image's rows); tests/test_gemm_route_cpu.py walks the same tables without a GPU.

Hardware observation (MI355X): v_mfma_scale_f32_16x16x128_f8f6f4 and v_mfma_f32_16x16x32_f16 accumulate these dot products
exactly -- every case below is bit-equal to the host's result."""
import pytest

pytestmark = pytest.mark.gpu

_VALUES = [0, 0, 0, 0, 0, 0, 1, -1, 2, -2, 3, -3, 4, -4, 6, -6]
_CACHE = {}         # operands of the current shape, built once (the host FP4 packing dominates) and shared by its cases


def _cache_scope(shape):
    """keep the operands of one shape at a time: the cases are ordered by shape"""
    if _CACHE.get("shape") != shape:
        _CACHE.clear()
        _CACHE["shape"] = shape


def _ints(seed, rows, cols):
    """float32 [rows][cols] of _VALUES; ~5 % of the 32-blocks all zero, ~5 % with a single non-zero"""
    import torch
    g = torch.Generator().manual_seed(seed)
    table = torch.tensor(_VALUES, dtype=torch.float32)
    x = table[torch.randint(0, 16, (rows, cols), generator=g)].reshape(rows, cols // 32, 32)
    u = torch.rand((rows, cols // 32, 1), generator=g)
    one = torch.randint(0, 32, (rows, cols // 32, 1), generator=g) == torch.arange(32).view(1, 1, 32)
    x = torch.where(u < 0.05, torch.zeros(()), torch.where((u < 0.10) & ~one, torch.zeros(()), x))
    return x.reshape(rows, cols)


def _q4(x, what):
    """(FP4 plane, scales) of float32 [rows][c] through the host quantiser; the values must survive it unchanged"""
    import torch
    from vision_semantic_segmentation_amd.network import mx_dequant_fp4, mx_quant_fp4
    q, s = mx_quant_fp4(x.double())
    assert torch.equal(mx_dequant_fp4(q, s), x.double()), "%s does not pass through FP4 unchanged" % what
    return q, s


def _pad(t, rows):
    import torch
    out = torch.zeros((rows,) + tuple(t.shape[1:]), dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


def _act(M, K, seed):
    """One MX GEMM input: f16 plane A, the values B and C of its bundle's halves, the bundle (rows padded to 256)"""
    key = ("act", M, K, seed)
    if key not in _CACHE:
        import torch
        Mp = (M + 255) // 256 * 256
        g = torch.Generator().manual_seed(seed + 5)
        A = _ints(seed, M, K)
        B = _ints(seed + 1, M, K) * torch.exp2(torch.randint(-1, 2, (M, 1), generator=g).float())
        Cc = _ints(seed + 2, M, K) * torch.exp2(torch.randint(-1, 2, (M, 1), generator=g).float())
        parts = []
        for t, nm in ((B, "B"), (Cc, "C")):
            q, s = _q4(_pad(t, Mp), nm)
            parts += [q.reshape(-1), s.reshape(-1)]
        _CACHE[key] = (A, B, Cc, _pad(A, Mp).to(torch.float16), torch.cat(parts))
    return _CACHE[key]


def _mx_weights(N, K, seed):
    """Wh (f16 rows), Wl and Wh' (the halves of w_mx, scales in the kernel's per-lane order), integer bias"""
    key = ("w", N, K, seed)
    if key not in _CACHE:
        import torch
        from vision_semantic_segmentation_amd.network import permute_w_scales
        Wh, Wl, Wh2 = _ints(seed, N, K), _ints(seed + 1, N, K), _ints(seed + 2, N, K)
        parts = []
        for t, nm in ((Wl, "Wl"), (Wh2, "Wh'")):
            q, s = _q4(t, nm)
            parts += [q.reshape(-1), permute_w_scales(s).reshape(-1)]
        _CACHE[key] = (Wh, Wl, Wh2, Wh.to(torch.float16), torch.cat(parts), _bias(N, seed + 3))
    return _CACHE[key]


def _bias(N, seed):
    """integers; every fourth column (shuffled) beyond +-2048, where the hi plane rounds and the lo part is non-zero"""
    import torch
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(-40, 41, (N,), generator=g).float()
    big = (2048 + torch.randint(0, 2000, (N,), generator=g)).float() * (torch.randint(0, 2, (N,), generator=g) * 2 - 1).float()
    return torch.where(torch.randint(0, 4, (N,), generator=g) == 0, big, b)


def _residual(M, N, seed):
    """integer f16 hi plane (|.| <= 1000), integer lo values (FP4-exact, so they serve as an f16 lo plane and as Q4(lo) alike)"""
    key = ("r", M, N, seed)
    if key not in _CACHE:
        import torch
        g = torch.Generator().manual_seed(seed)
        _CACHE[key] = (torch.randint(-1000, 1001, (M, N), generator=g).float(), _ints(seed + 1, M, N))
    return _CACHE[key]


def _expect(acc, relu):
    """exact result v (float64) -> (v, f16 hi plane, fp32 v - hi, f16 lo plane)"""
    import torch
    v = torch.relu(acc) if relu else acc
    hi = v.to(torch.float16)
    lo32 = (v - hi.double()).float()
    assert torch.equal(lo32.double(), v - hi.double())
    return v, hi, lo32, lo32.to(torch.float16)


def _gemm_op(M, K, N, Mp, relu, batch=0, hw=None):
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_GEMM, AvlSegOp
    op = AvlSegOp()
    op.kind, op.dtype = OP_GEMM, _lib.AVL_F16
    h, w = hw if hw else (1, M)
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = h, w, K, K, Mp
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = h, w, N, N, Mp
    op.relu, op.ksize, op.stride, op.dil, op.groups, op.batch = int(relu), 1, 1, 1, 1, batch
    return op


def _same_values(got, want):
    """two float tensors hold the same values everywhere (+0 == -0; no NaN expected)"""
    import torch
    return got.shape == want.shape and bool(torch.equal(got, want))


# (M, K, K2, N, form, relu, the kernel the op runs): K2 = columns of a second input appended along K; forms
#   plain = weights-only correction, no residual, one output plane                                   (IO 0)
#   noq   = in_lo, single-plane residual, split output, no out_mx                                    (IO 0)
#   split = in_lo, split f16 residual, split output, out_mx with both halves                         (IO 1)
#   hiq   = weights-only correction, no residual, one output plane, out_mx with its hi half only     (IO 1)
#   trunk = AVL_MX_IN_LO | AVL_MX_RES_LO | AVL_MX_OUT_LO: every lo part only as FP4                  (IO 1)
MX_CASES = [
    # 256-row tiles: N = 2048, M = 5900 -> 24 row tiles (the last holds 12 rows), t256 = 24 * 8 = 192
    (5900, 256, 0, 2048, "plain", True, "k_gemm_ring_mx<0, 8>"),      # one macro-block
    (5900, 256, 0, 2048, "split", False, "k_gemm_ring_mx<1, 8>"),
    (5900, 256, 0, 2048, "trunk", True, "k_gemm_ring_mx<1, 8>"),
    (5900, 1024, 0, 2048, "noq", False, "k_gemm_mx_pipe<0, 8, 0>"),      # K = 1024
    (5900, 1024, 0, 2048, "split", True, "k_gemm_mx_pipe<1, 8, 0>"),
    (5900, 1024, 0, 2048, "trunk", False, "k_gemm_mx_pipe<1, 8, 0>"),
    (5900, 1280, 0, 2048, "plain", False, "k_gemm_mx_pipe<0, 8, 0>"),      # odd macro-block count (5)
    (5900, 1280, 0, 2048, "hiq", True, "k_gemm_mx_pipe<1, 8, 0>"),
    (5900, 1280, 0, 2048, "trunk", True, "k_gemm_mx_pipe<1, 8, 0>"),
    # more tiles than CUs, a workgroup walks several: M = 12100 -> t256 = 48 * 8 = 384: 256-row tiles, 384 of them
    (12100, 1024, 0, 2048, "trunk", True, "k_gemm_mx_pipe<1, 8, 0>"),
    # 128-row tiles: t256 = 2 * 1 = 2 and 4 * 2 = 8
    (300, 256, 0, 256, "plain", False, "k_gemm_ring_mx<0, 4>"),
    (300, 1024, 0, 256, "split", True, "k_gemm_mx_pipe<1, 4, 1>"),
    (777, 256, 0, 512, "trunk", False, "k_gemm_ring_mx<1, 4>"),
    (777, 256, 0, 512, "split", True, "k_gemm_ring_mx<1, 4>"),
    (777, 1024, 0, 512, "noq", True, "k_gemm_mx_pipe<0, 4, 1>"),
    (777, 1024, 0, 512, "trunk", True, "k_gemm_mx_pipe<1, 4, 1>"),
    # 128-row tiles again above 256: M = 8300 -> t256 = 33 * 8 = 264, 65 * 8 = 520 tiles of 128 rows on 256 workgroups
    (8300, 256, 0, 2048, "trunk", True, "k_gemm_ring_mx<1, 4>"),
    # a second input along K, 128-row tiles (t256 = 8)
    (777, 256, 512, 512, "trunk", True, "k_gemm_ring_mx<1, 4>"),      # K1 + K2 = 768: the input changes after macro-block 1 of 3
    (777, 512, 512, 512, "trunk", False, "k_gemm_mx_pipe<1, 4, 1>"),      # K1 + K2 = 1024: the input changes in the middle of the stream
    # ... and 256-row tiles (t256 = 192)
    (5900, 256, 512, 2048, "trunk", False, "k_gemm_ring_mx<1, 8>"),
    (5900, 512, 512, 2048, "trunk", True, "k_gemm_mx_pipe<1, 8, 0>"),
    (5900, 512, 768, 2048, "noq", True, "k_gemm_mx_pipe<0, 8, 0>"),      # plain in_lo is refused with a second input, so AVL_MX_IN_LO
]


def _mx_form(form):
    """-> (correction passes, the residual's form, split output, out_mx set, the bundle's lo half is written)"""
    return (1 if form in ("plain", "hiq") else 2, {"plain": None, "hiq": None, "noq": "single", "split": "split", "trunk": "fp4"}[form],
            form in ("noq", "split"), form in ("split", "hiq", "trunk"), form in ("split", "trunk"))


def mx_shape_op(case, ptr, batch=0, hw=None):
    """the case's op with `ptr` (16-byte aligned) in every pointer field its form sets: all that the library's validation and its
    choice of kernel look at.  _run_mx puts the device buffers in; tests/test_gemm_route_cpu.py asks for the route as it stands."""
    from vision_semantic_segmentation_amd.network import AVL_MX_IN_LO, AVL_MX_OUT_LO, AVL_MX_RES_LO
    M, K1, K2, N, form, relu = case[:6]
    nmx, res, o_split, quant, _ = _mx_form(form)
    op = _gemm_op(M if not batch else hw[0] * hw[1], K1, N, (M + 255) // 256 * 256, relu, batch, hw)
    op.in_ = op.out = op.weight = op.bias = op.w_mx = op.in_mx = ptr
    op.w_rows, op.w_split = N, 2
    flags = 0
    if nmx == 2:
        if form == "trunk" or K2:
            flags |= AVL_MX_IN_LO
        else:
            op.in_lo = ptr                                       # switches the second pass on; its values are never read
    if K2:
        op.in3, op.in3_mx, op.in3_c, op.in3_ld = ptr, ptr, K2, K2
    if o_split:
        op.out_lo = ptr
    if quant:
        op.out_mx = ptr
        if form == "trunk":
            flags |= AVL_MX_OUT_LO
    if res:
        op.in2, op.in2_ld = ptr, N
        if res == "split":
            op.in2_lo = ptr
        if res == "fp4":
            op.in2_mx = ptr
            flags |= AVL_MX_RES_LO
    op.mx_flags = flags
    return op


def _run_mx(case, cuda_device, batch=0, hw=None):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import gemm_kernel_name, gemm_route, mx_bundle_bytes, mx_quant_fp4
    M, K1, K2, N, form, relu, kernel = case
    K, Mp = K1 + K2, (M + 255) // 256 * 256
    assert 216 * K <= 2 ** 19                                   # the exactness bound of the module docstring
    seed = 1000 * (M % 97) + K1 + 3 * K2 + N
    _cache_scope((M, K1, K2, N))
    ins = [_act(M, K1, seed)] + ([_act(M, K2, seed + 50)] if K2 else [])
    Wh, Wl, Wh2, w16, wmx, bias = _mx_weights(N, K, seed + 100)
    nmx, res, o_split, quant, lo_half = _mx_form(form)
    # expected accumulator: one exact fp32 product over the concatenated K ranges
    cat = lambda i: torch.cat([t[i] for t in ins], dim=1)       # noqa: E731
    acc = cat(0) @ Wh.t() + cat(1) @ Wl.t() + bias
    if nmx == 2:
        acc = acc + cat(2) @ Wh2.t()
    acc = acc.double()
    if res:
        r_hi, r_lo = _residual(M, N, seed + 200)
        acc = acc + r_hi.double() + (r_lo.double() if res != "single" else 0)
    v, hi, lo32, lo16 = _expect(acc, relu)
    assert float(v.abs().max()) > 2048 and bool((lo32 != 0).any())
    if not relu:
        assert 0.3 < float((v < 0).double().mean()) < 0.7

    dev = [(a[3].to(cuda_device), a[4].to(cuda_device)) for a in ins]
    wd, wmxd, bd = w16.to(cuda_device), wmx.to(cuda_device), bias.to(cuda_device)
    out = torch.full((2, Mp, N), 7.0, dtype=torch.float16, device=cuda_device)
    hb = mx_bundle_bytes(Mp, N)
    out_mx = torch.full((2 * hb,), 0xEE, dtype=torch.uint8, device=cuda_device)
    op = mx_shape_op(case, 16, batch, hw)                       # every pointer field the form sets, then the device buffers in them
    op.in_, op.out, op.weight, op.bias = dev[0][0].data_ptr(), out[0].data_ptr(), wd.data_ptr(), bd.data_ptr()
    op.w_mx, op.in_mx = wmxd.data_ptr(), dev[0][1].data_ptr()
    if op.in_lo:
        nan_plane = torch.full((Mp, K1), float("nan"), dtype=torch.float16, device=cuda_device)
        op.in_lo = nan_plane.data_ptr()                          # switches the second pass on; its values are never read
    if K2:
        op.in3, op.in3_mx = dev[1][0].data_ptr(), dev[1][1].data_ptr()
    if o_split:
        op.out_lo = out[1].data_ptr()
    if quant:
        op.out_mx = out_mx.data_ptr()
    if res:
        rd = torch.stack([_pad(r_hi, Mp), _pad(r_lo, Mp)]).to(torch.float16).to(cuda_device)
        op.in2 = rd[0].data_ptr()
        if res == "split":
            op.in2_lo = rd[1].data_ptr()
        if res == "fp4":
            g = torch.Generator().manual_seed(seed)
            q, s = _q4(_pad(r_lo, Mp), "residual lo")
            r_mx = torch.cat([torch.randint(0, 256, (hb,), generator=g, dtype=torch.uint8), q.reshape(-1), s.reshape(-1)]).to(cuda_device)
            op.in2_mx = r_mx.data_ptr()                          # hi half: random bytes the kernel must not read
    assert gemm_kernel_name(gemm_route(op)) == kernel, case     # the kernel this case is here for, on the op that runs
    _run_plan([op])

    o = out.cpu()
    bad = int((o[0, :M] != hi).sum())
    assert _same_values(o[0, :M], hi), "hi plane: %d of %d values differ, max |diff| %g" % (bad, hi.numel(), float((o[0, :M].double() - hi.double()).abs().max()))
    assert torch.all(o[0, M:] == 7.0)
    if o_split:
        assert _same_values(o[1, :M], lo16), "lo plane: %d values differ" % int((o[1, :M] != lo16).sum())
        assert torch.all(o[1, M:] == 7.0)
    else:
        assert torch.all(o[1] == 7.0)                           # no f16 lo plane is written
    b = out_mx.cpu()
    if not quant:
        assert torch.all(b == 0xEE)
        return
    for half, want in ((0, hi.double()), (1, (lo16 if o_split else lo32).double())):
        hbuf = b[half * hb:(half + 1) * hb]
        qd, sd = hbuf[:Mp * (N // 2)].reshape(Mp, N // 2), hbuf[Mp * (N // 2):].reshape(N // 256, Mp, 8)
        if half == 1 and not lo_half:
            assert torch.all(hbuf == 0xEE)                      # the lo half is not written
            continue
        qr, sr = mx_quant_fp4(want)
        assert torch.equal(sd[:, :M], sr), "out_mx half %d: %d scale bytes differ" % (half, int((sd[:, :M] != sr).sum()))
        assert torch.equal(qd[:M], qr), "out_mx half %d: %d FP4 bytes differ" % (half, int((qd[:M] != qr).sum()))
        assert torch.all(qd[M:] == 0xEE) and torch.all(sd[:, M:] == 0xEE)      # rows past M: plane and every scale slab


@pytest.mark.parametrize("case", MX_CASES, ids=lambda c: "%d-%d+%d-%d-%s-%d" % c[:6])
def test_mx_gemm_exact(case, cuda_device):
    _run_mx(case, cuda_device)


BATCH_CASE = (778, 1024, 0, 512, "trunk", True, "k_gemm_mx_pipe<1, 4, 1>")


def test_mx_gemm_exact_batch_of_two(cuda_device):
    """batch = 2, 389 pixels per image: the image boundary falls inside the fourth 128-row tile.  Images are packed densely and the
    bundles keep the plain layout (image n at row offset n * 389 of each plane and slab, slab stride = all rows: the BATCH paragraph
    of include/avl_hip.h), so the expected bytes are those of one 778-row GEMM.  t256 is counted on one image: 2 * 2 = 4,
    128-row tiles, K = 1024."""
    _run_mx(BATCH_CASE, cuda_device, batch=2, hw=(1, 389))


# (M, K, N, nsub, residual, split output, relu)
SPLIT_CASES = [(M, K, N, nsub, res, osp, (i + nsub) % 2 == 0)
               # t256 = 11 * 1 = 11: the 256 x 128 ring; t256 = 24 * 8 = 192: the 256 x 256 ring.  K = 192: three 64-wide blocks
               for M, K, N in ((2600, 192, 256), (5900, 192, 2048))
               for nsub in (2, 3)
               for i, (res, osp) in enumerate(((None, False), (None, True), ("single", True), ("split", False)))]


# (N, nsub) -> the kernel a split case runs: <f16, WM, WN, MI, STAGES, NSUB, IO, AST, EXT>
SPLIT_KERNELS = {(256, 2): "k_gemm_ring<f16, 4, 2, 4, 3, 2, 1, 3, false>", (256, 3): "k_gemm_ring<f16, 4, 2, 4, 3, 3, 1, 3, false>",
                 (2048, 2): "k_gemm_ring<f16, 2, 4, 8, 3, 2, 1, 2, false>", (2048, 3): "k_gemm_ring<f16, 2, 4, 8, 2, 3, 1, 2, false>"}


def split_shape_op(case, ptr):
    """the split case's op with `ptr` in every pointer field it sets (see mx_shape_op)"""
    M, K, N, nsub, res, o_split, relu = case
    op = _gemm_op(M, K, N, (M + 255) // 256 * 256, relu)
    op.in_ = op.out = op.weight = op.bias = ptr
    op.w_rows, op.w_split = N, 1
    if nsub == 3:
        op.in_lo = ptr
    if o_split:
        op.out_lo = ptr
    if res:
        op.in2, op.in2_ld = ptr, N
        if res == "split":
            op.in2_lo = ptr
    return op


def _split_weights(N, K, nsub, seed, rows):
    """f16 [rows][K/64][W1 64 | W2 64 (| W3 64)] from independent matrices (the order of network.pack_split_rows, whose blocks are
    hi | lo (| hi)); rows past N hold values too: they must reach no output"""
    import torch
    ws = [_ints(seed + j, rows, K) for j in range(nsub)]
    packed = torch.cat([w.reshape(rows, K // 64, 1, 64) for w in ws], dim=2).reshape(rows, K * nsub)
    return ws, packed.to(torch.float16).contiguous()


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: "%d-%d-%d-nsub%d-res_%s-split%d-relu%d" % c)
def test_split_gemm_exact(case, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import gemm_kernel_name, gemm_route
    M, K, N, nsub, res, o_split, relu = case
    Mp = (M + 255) // 256 * 256
    seed = 7000 + M + N + nsub
    A, A_lo = _ints(seed, M, K), _ints(seed + 10, M, K)
    ws, packed = _split_weights(N, K, nsub, seed + 20, N)
    bias = _bias(N, seed + 30)
    acc = A @ ws[0].t() + A @ ws[1].t() + bias
    if nsub == 3:
        acc = acc + A_lo @ ws[2].t()
    acc = acc.double()
    if res:
        r_hi, r_lo = _residual(M, N, seed + 40)
        acc = acc + r_hi.double() + (r_lo.double() if res == "split" else 0)
    v, hi, lo32, lo16 = _expect(acc, relu)
    assert float(v.abs().max()) > 2048 and bool((lo32 != 0).any())
    planes = torch.stack([_pad(A, Mp), _pad(A_lo, Mp)]).to(torch.float16).to(cuda_device)
    wd, bd = packed.to(cuda_device), bias.to(cuda_device)
    out = torch.full((2, Mp, N), 7.0, dtype=torch.float16, device=cuda_device)
    op = split_shape_op(case, 16)
    op.in_, op.out, op.weight, op.bias = planes[0].data_ptr(), out[0].data_ptr(), wd.data_ptr(), bd.data_ptr()
    if nsub == 3:
        op.in_lo = planes[1].data_ptr()
    if o_split:
        op.out_lo = out[1].data_ptr()
    if res:
        rd = torch.stack([_pad(r_hi, Mp), _pad(r_lo, Mp)]).to(torch.float16).to(cuda_device)
        op.in2 = rd[0].data_ptr()
        if res == "split":
            op.in2_lo = rd[1].data_ptr()
    assert gemm_kernel_name(gemm_route(op)) == SPLIT_KERNELS[(N, nsub)], case
    _run_plan([op])
    o = out.cpu()
    assert _same_values(o[0, :M], hi), "hi plane: %d of %d values differ" % (int((o[0, :M] != hi).sum()), hi.numel())
    assert torch.all(o[0, M:] == 7.0)
    if o_split:
        assert _same_values(o[1, :M], lo16), "lo plane: %d values differ" % int((o[1, :M] != lo16).sum())
        assert torch.all(o[1, M:] == 7.0)
    else:
        assert torch.all(o[1] == 7.0)


@pytest.mark.parametrize("M", [777, 300])
def test_split_classifier_exact(M, cuda_device):
    """The classifier form: N = 19, fp32 output, nsub 3, in the small-N kernel (asserted below).  Exact in fp32; the
    45 weight rows past N hold values and reach nothing; out_ld = 19, so a stray column would land in the next row."""
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import gemm_kernel_name, gemm_route
    K, N, rows = 256, 19, 64
    Mp = (M + 255) // 256 * 256
    seed = 9000 + M
    A, A_lo = _ints(seed, M, K), _ints(seed + 10, M, K)
    ws, packed = _split_weights(N, K, 3, seed + 20, rows)
    bias = torch.zeros(rows)
    bias[:N] = _bias(N, seed + 30)
    bias[N:] = 12345.0
    want = (A @ ws[0][:N].t() + A @ ws[1][:N].t() + A_lo @ ws[2][:N].t() + bias[:N]).double()
    planes = torch.stack([_pad(A, Mp), _pad(A_lo, Mp)]).to(torch.float16).to(cuda_device)
    wd, bd = packed.to(cuda_device), bias.to(cuda_device)
    out = torch.full((Mp, N), -7.0, dtype=torch.float32, device=cuda_device)
    op = _gemm_op(M, K, N, Mp, False)
    op.in_, op.in_lo, op.out, op.weight, op.bias = planes[0].data_ptr(), planes[1].data_ptr(), out.data_ptr(), wd.data_ptr(), bd.data_ptr()
    op.w_rows, op.w_split, op.out_f32 = rows, 1, 1
    assert gemm_kernel_name(gemm_route(op)) == "k_gemm<f16, 4, 1>"
    _run_plan([op])
    o = out.cpu()
    assert torch.equal(o[:M].double(), want), "%d logits differ" % int((o[:M].double() != want).sum())
    assert torch.all(o[M:] == -7.0)
