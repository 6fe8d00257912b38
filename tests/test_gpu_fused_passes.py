"""The ring GEMM's two extra forms (SegNet(fuse_passes=True)), each run ALONE through avl_seg_plan_* and compared bit for bit with the
stand-alone ops it replaces, then the whole plan with the keyword on against off.

  strided rows        a stride-s 1x1 conv reads every s-th pixel of every s-th row itself; reference = AVL_OP_SUBSAMPLE (one launch per
                      plane) into a compact buffer, then the plain GEMM on it.
  second destination  two 1x1 convs of one input in one launch; reference = the two single-destination GEMMs.

Nothing is rounded differently: the same products are accumulated in the same order, so every comparison is torch.equal on whole
buffers -- the fill pattern of rows and columns the op must not touch included.

(tests/test_gpu_ring_ext_exact.py compares the same forms with a float64 host reference, at sizes where a workgroup walks several
tiles.)  The whole-plan tests also compare the per-op non-finite counts, op by op, and the flops / bytes SegNet.profile() reports."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

FILL = 7.0
K = 256


def _gemm(did, src, src_lo, w, b, dst, dst_lo, in_hw, out_hw, n, in_ld, out_ld, in_rows, out_rows, batch, **f):
    from vision_semantic_segmentation_amd.network import OP_GEMM, AvlSegOp
    op = AvlSegOp()
    op.kind, op.dtype = OP_GEMM, did
    op.in_, op.out, op.weight, op.bias = src, dst, w.data_ptr(), b.data_ptr()
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = in_hw[0], in_hw[1], K, in_ld, in_rows
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = out_hw[0], out_hw[1], n, out_ld, out_rows
    op.relu, op.w_rows, op.ksize, op.stride, op.dil, op.groups, op.batch = 1, w.shape[0], 1, 1, 1, 1, batch
    if src_lo or dst_lo:
        op.w_split, op.in_lo, op.out_lo = 1, src_lo, dst_lo
    for k, v in f.items():
        setattr(op, k, v)
    return op


def _runs_ext_ring(op, mode, w_layout):
    """the op runs the EXT instantiation of the ring kernel that tests/_ring_ext_operands.py names for its mode and tile variant
    (w_layout 3 = 256 x 256 tiles; by shape these sizes run 256 x 128): asked of the library for the very op"""
    import _ring_ext_operands as R
    from vision_semantic_segmentation_amd.network import gemm_kernel_name, gemm_route
    assert gemm_kernel_name(gemm_route(op)) == "k_gemm_ring<%s>" % R.INSTANTIATION[(mode, w_layout or 2)]


def _operands(mode, n, rows, ld, seed, cuda_device):
    """input planes [2 | 1][rows][ld] (NaN outside the K columns that are read), packed weights [round_up(n, 256)][..], bias"""
    import torch
    from vision_semantic_segmentation_amd.network import pack_split_rows
    tdt = torch.bfloat16 if mode == "bf16" else torch.float16
    g = torch.Generator().manual_seed(seed)
    planes = 2 if mode == "split" else 1
    a = torch.full((planes, rows, ld), float("nan"), dtype=tdt)
    a[0, :, :K] = torch.randn((rows, K), generator=g).to(tdt)
    if planes == 2:
        a[1, :, :K] = (torch.randn((rows, K), generator=g) * 2 ** -12).to(tdt)
    w_rows = (n + 255) // 256 * 256
    w64 = torch.zeros((w_rows, K), dtype=torch.float64)
    w64[:n] = torch.randn((n, K), generator=g, dtype=torch.float64) / K ** 0.5
    b = torch.zeros(w_rows)
    b[:n] = torch.randn(n, generator=g)
    # "split": input and weights as f16 pairs (three passes); "w2": weights only (two passes); else one plane of the type
    pack = {"split": lambda m: pack_split_rows(m, 3), "w2": lambda m: pack_split_rows(m, 2)}.get(mode, lambda m: m.to(tdt))
    return a.to(cuda_device), w64, b, pack, tdt


def _did(mode):
    from vision_semantic_segmentation_amd import _lib
    return _lib.AVL_BF16 if mode == "bf16" else _lib.AVL_F16


@pytest.mark.parametrize("case", [  # (in_h, in_w, mode, batch, extra input row stride)
    (9, 13, "split", 1, 0),         # 5 x 7 = 35 rows: one tile, mostly padding
    (20, 36, "split", 1, 0),        # 180 rows: one partial tile
    (46, 60, "split", 1, 0),        # 690 rows: three tiles, the last partial
    (46, 60, "f16", 1, 0),
    (20, 36, "bf16", 1, 0),
    (20, 36, "split", 2, 0),        # image 1's pixels start at row in_h * in_w of the input, inside a row tile of the output
    (9, 13, "f16", 1, 64),          # input rows wider than K
    # w_layout 3: the 256 x 256 tile the 1080p plans run (w_layout 0 picks 256 x 128 at these sizes), three, two and one pass
    (46, 60, "split", 1, 0, 3),
    (46, 60, "w2", 1, 0, 3),
    (20, 36, "f16", 2, 0, 3),
    (20, 36, "bf16", 1, 0, 3),
])
def test_strided_gemm_equals_subsample_then_gemm(case, cuda_device):
    import torch
    from test_gpu_ops import _run_plan, _spatial_op
    from vision_semantic_segmentation_amd.network import OP_SUBSAMPLE
    ih, iw, mode, B, extra = case[:5]
    kw = dict(w_layout=case[5]) if len(case) > 5 else {}
    if mode == "w2":
        kw["w_split"] = 1
    s, N = 2, 512
    oh, ow = (ih - 1) // s + 1, (iw - 1) // s + 1
    in_rows, out_rows = (B * ih * iw + 255) // 256 * 256, (B * oh * ow + 255) // 256 * 256
    ld = K + extra
    did = _did(mode)
    a, w64, b, pack, tdt = _operands(mode, N, in_rows, ld, 5, cuda_device)
    a[:, B * ih * iw:] = float("nan")              # rows past the last image: never part of a stored result
    wd, bd = pack(w64).to(cuda_device), b.to(cuda_device)
    planes = a.shape[0]
    lo = lambda t: t[1].data_ptr() if planes == 2 else 0

    compact = torch.zeros((planes, out_rows, K), dtype=tdt, device=cuda_device)
    ref = torch.full((planes, out_rows, N), FILL, dtype=tdt, device=cuda_device)
    ops = [_spatial_op(OP_SUBSAMPLE, did, a[p], (ih, iw), K, compact[p], (oh, ow), K, stride=s, batch=B) for p in range(planes)]
    ops.append(_gemm(did, compact[0].data_ptr(), lo(compact), wd, bd, ref[0].data_ptr(), lo(ref), (oh, ow), (oh, ow), N, K, N, out_rows, out_rows, B, **kw))
    _run_plan(ops)

    got = torch.full((planes, out_rows, N), FILL, dtype=tdt, device=cuda_device)
    strided = _gemm(did, a[0].data_ptr(), lo(a), wd, bd, got[0].data_ptr(), lo(got), (ih, iw), (oh, ow), N, ld, N, in_rows, out_rows, B, stride=s, **kw)
    _runs_ext_ring(strided, mode, kw.get("w_layout"))
    _run_plan([strided])
    assert bool(torch.isfinite(ref[:, :B * oh * ow].float()).all()) and float(ref[0, :B * oh * ow].float().abs().max()) > 0
    for p in range(planes):
        assert torch.equal(got[p], ref[p]), "%r: plane %d differs from sub-sample -> GEMM" % (case, p)
    assert bool((got[:, B * oh * ow:] == FILL).all())


@pytest.mark.parametrize("case", [  # (first conv's columns, second's, mode)
    (256, 256, "split"),            # the network's op: N = 512
    (128, 256, "split"),            # LOW_LEVEL_OUT_CHANNELS padded to 128: N = 384, the 128-wide N tile
    (256, 256, "f16"),
    (128, 256, "bf16"),
    # w_layout 3: the 256 x 256 tile of the 1080p plans (n_split = one N tile), three, two and one pass
    (256, 256, "split", 3),
    (256, 256, "w2", 3),
    (256, 256, "f16", 3),
    (256, 256, "bf16", 3),
])
def test_twin_gemm_equals_two_gemms(case, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    n1, n2, mode = case[:3]
    kw = dict(w_layout=case[3]) if len(case) > 3 else {}
    if mode == "w2":
        kw["w_split"] = 1
    M, rows = 300, 512
    did = _did(mode)
    a, w64, b, pack, tdt = _operands(mode, n1 + n2, rows, K, 9, cuda_device)
    a[:, M:] = float("nan")
    planes = a.shape[0]
    lo = lambda t, col=0: t[1, :, col:].data_ptr() if planes == 2 else 0
    w_rows = w64.shape[0]

    def part(r0, n):               # the rows of one conv alone, padded as a plan pads them
        w = torch.zeros(((n + 255) // 256 * 256, K), dtype=torch.float64)
        w[:n] = w64[r0:r0 + n]
        bb = torch.zeros(w.shape[0])
        bb[:n] = b[r0:r0 + n]
        return pack(w).to(cuda_device), bb.to(cuda_device)

    col = 256                      # the first destination: columns col .. col + n1 of a 512-wide buffer; the second: a single 256-wide plane
    new = lambda: (torch.full((planes, rows, 512), FILL, dtype=tdt, device=cuda_device), torch.full((rows, 256), FILL, dtype=tdt, device=cuda_device))
    ref1, ref2 = new()
    (w1, b1), (w2, b2) = part(0, n1), part(n1, n2)
    _run_plan([_gemm(did, a[0].data_ptr(), lo(a), w1, b1, ref1[0, :, col:].data_ptr(), lo(ref1, col), (1, M), (1, M), n1, K, 512, rows, rows, 1, **kw),
               _gemm(did, a[0].data_ptr(), lo(a), w2, b2, ref2.data_ptr(), 0, (1, M), (1, M), n2, K, 256, rows, rows, 1,
                     **dict(kw, **(dict(w_split=1) if planes == 2 else {})))])
    assert bool(torch.isfinite(ref2[:M].float()).all()) and float(ref2[:M].float().abs().max()) > 0

    wd, bd = pack(w64).to(cuda_device), b.to(cuda_device)
    assert wd.shape[0] == w_rows
    got1, got2 = new()
    twin = _gemm(did, a[0].data_ptr(), lo(a), wd, bd, got1[0, :, col:].data_ptr(), lo(got1, col), (1, M), (1, M), n1 + n2, K, 512, rows, rows, 1,
                 out2=got2.data_ptr(), out2_ld=256, n_split=n1, **kw)
    _runs_ext_ring(twin, mode, kw.get("w_layout"))
    first = None
    for rep in range(3):           # a race screen: the same bytes every time
        _run_plan([twin])
        assert torch.equal(got1, ref1), "%r, launch %d: first destination differs from its own GEMM" % (case, rep)
        assert torch.equal(got2, ref2), "%r, launch %d: second destination differs from its own GEMM" % (case, rep)
        snap = (got1.clone(), got2.clone())
        assert first is None or (torch.equal(snap[0], first[0]) and torch.equal(snap[1], first[1]))
        first = first or snap
        got1.fill_(FILL)
        got2.fill_(FILL)
    assert bool((ref1[:, :, :col] == FILL).all()) and bool((ref1[:, M:] == FILL).all()) and bool((ref1[:, :, col + n1:] == FILL).all())
    assert bool((ref2[M:] == FILL).all())


MERGED, POOLED_STEM, DOWNSAMPLE = "backbone.layer2.0.conv1+decoder.low_level_conv", "backbone.conv1+maxpool", "backbone.layer2.0.downsample"
# what each fused op replaces in the plan built with fuse_passes=False
REPLACES = {MERGED: ("backbone.layer2.0.conv1", "decoder.low_level_conv"), POOLED_STEM: ("backbone.conv1", "backbone.maxpool"),
            DOWNSAMPLE: (DOWNSAMPLE + ".sub", DOWNSAMPLE + ".sub[lo]", DOWNSAMPLE)}


def _unfused_view(counts):
    """per-op non-finite counts of an unfused plan under the fused plan's op names: a merged op's outputs are those of the two
    ops it replaces; the pooled stem writes the max-pool's map only; the sub-sampled copies do not exist"""
    d = dict(counts)
    merged = d.pop("backbone.layer2.0.conv1", 0) + d.pop("decoder.low_level_conv", 0)
    if merged:
        d[MERGED] = merged
    d.pop("backbone.conv1", None)
    if d.get("backbone.maxpool"):
        d[POOLED_STEM] = d["backbone.maxpool"]
    d.pop("backbone.maxpool", None)
    d.pop(DOWNSAMPLE + ".sub", None)
    d.pop(DOWNSAMPLE + ".sub[lo]", None)
    return d


# ("mixed", 512, 516): layer1's output is 128 x 129 = 16 512 rows, so the merged op itself has 65 row tiles x 4 N tiles = 260 > 256
@pytest.mark.parametrize("case", [("mixed", 97, 131), ("mixed", 192, 256), ("f16", 97, 131), ("bf16", 97, 131), ("mixed", 512, 516)])
def test_whole_plan_is_unchanged_by_fuse_passes(case, cuda_device):
    import torch
    from vision_semantic_segmentation_amd.network import SegNet, random_state_dict
    precision, H, W = case
    st = random_state_dict(seed=0)
    img = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(cuda_device)
    outs = []
    for fuse in (True, False):
        net = SegNet(st, H, W, precision=precision, device=cuda_device, fuse_passes=fuse)
        assert (MERGED in net.op_names) == fuse
        assert ("backbone.layer2.0.downsample.sub" in net.op_names) != fuse
        if (H, W) == (512, 516):
            op = net.ops[net.op_names.index(MERGED if fuse else "backbone.layer2.0.conv1")]
            assert op.out_h * op.out_w == 16512 and (not fuse or (op.out2 and (16512 + 255) // 256 * (op.out_c // 128) > 256))
        net.forward(img)
        torch.cuda.synchronize()
        outs.append((net.logits.clone(), net.labels.clone(), net.nonfinite_counts()))
    assert bool(torch.isfinite(outs[0][0]).all())
    assert torch.equal(outs[0][0], outs[1][0]), "%r: logits differ" % (case,)
    assert torch.equal(outs[0][1], outs[1][1]), "%r: labels differ" % (case,)
    assert outs[0][2] == _unfused_view(outs[1][2]), (outs[0][2], outs[1][2])         # per-op counts, as dictionaries


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_whole_plan_counts_an_overflow_in_the_same_ops(precision, cuda_device):
    """the comparison above on counts that are NOT zero: a checkpoint whose folded BN bias is +Inf on one channel of
    decoder.low_level_conv (the merged op's first destination) and one of layer2.0.conv1 (its second), both under a ReLU.  The
    merged op counts one value per pixel and poisoned channel -- known from the operands -- and every op behind it counts what its
    unfused twin counts."""
    import torch
    from vision_semantic_segmentation_amd.network import SegNet, random_state_dict
    H, W = 97, 131
    st = {k: v.clone() for k, v in random_state_dict(seed=0).items()}
    st["decoder.low_level_conv.bn.bias"][5] = float("inf")
    st["backbone.layer2.0.bn1.bias"][3] = float("inf")
    img = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(cuda_device)
    counts = {}
    for fuse in (True, False):
        net = SegNet(st, H, W, precision=precision, device=cuda_device, fuse_passes=fuse)
        net.forward(img)
        torch.cuda.synchronize()
        counts[fuse] = net.nonfinite_counts()
        if fuse:
            op = net.ops[net.op_names.index(MERGED)]
            assert op.out2 and counts[fuse][MERGED] == 2 * op.out_h * op.out_w
    assert "decoder.low_level_conv" in counts[False] and "backbone.layer2.0.conv1" in counts[False] and len(counts[True]) > 3
    assert counts[True] == _unfused_view(counts[False]), (counts[True], counts[False])


@pytest.mark.parametrize("precision", ["mixed", "bf16"])
def test_profile_accounts_the_same_work_with_and_without_fuse_passes(precision, cuda_device):
    """avl_seg_plan_profile's flops and bytes (the benchmark's roofline reads them through SegNet.profile()): a fused op does the
    flops of the ops it replaces and moves no more bytes than they do.  No timing is asserted."""
    from vision_semantic_segmentation_amd.network import SegNet, random_state_dict
    st = random_state_dict(seed=0)
    prof = {}
    for fuse in (True, False):
        net = SegNet(st, 97, 131, precision=precision, device=cuda_device, fuse_passes=fuse)
        rows = net.profile()
        assert len({r["name"] for r in rows}) == len(rows)
        prof[fuse] = {r["name"]: r for r in rows}
    on, off = prof[True], prof[False]
    assert sum(r["flops"] for r in on.values()) == sum(r["flops"] for r in off.values()) > 0
    for name, parts in REPLACES.items():
        assert name in on and all(p in off for p in parts if not p.endswith("[lo]")), name
        old = [off[p] for p in parts if p in off]
        assert on[name]["flops"] == sum(r["flops"] for r in old) > 0, name
        assert 0 < on[name]["bytes"] <= sum(r["bytes"] for r in old), (name, on[name]["bytes"], [r["bytes"] for r in old])
    assert on[MERGED]["flops"] == off["backbone.layer2.0.conv1"]["flops"] + off["decoder.low_level_conv"]["flops"]
    assert on[DOWNSAMPLE]["flops"] == off[DOWNSAMPLE]["flops"]                    # the sub-sampled copies do no flops
    assert on[POOLED_STEM]["flops"] == off["backbone.conv1"]["flops"]              # nor does the max-pool
    for name in on:                                                               # every other op is the same op
        if name not in REPLACES:
            assert on[name]["flops"] == off[name]["flops"] and on[name]["bytes"] == off[name]["bytes"], name


# ------------------------------------------------------------------------------------------------ the stem with the max-pool in its epilogue
def _stem_ops(did, img, wd, bd, stem, pool, fused, hw, batch, in_format=0):
    """(stem op -> max-pool op into `pool`, the pooled stem (stride 4) into `fused`) on the same image and weights"""
    from test_gpu_ops import _spatial_op
    from vision_semantic_segmentation_amd.network import OP_MAXPOOL, OP_STEM, AvlSegOp
    H, W = hw
    h2, w2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h4, w4 = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1

    def stem_op(dst, oh, ow, stride):
        op = AvlSegOp()
        op.kind, op.dtype = OP_STEM, did
        op.in_, op.out, op.weight, op.bias = img.data_ptr(), dst.data_ptr(), wd.data_ptr(), bd.data_ptr()
        op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = H, W, 3, 3, batch * H * W
        op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = oh, ow, 64, 64, dst.shape[0]
        op.ksize, op.stride, op.pad, op.dil, op.groups, op.relu, op.w_layout, op.batch, op.in_format = 7, stride, 3, 1, 1, 1, 1, batch, in_format
        return op
    mp = _spatial_op(OP_MAXPOOL, did, stem, (h2, w2), 64, pool, (h4, w4), 64, ksize=3, stride=2, pad=1, dil=1, batch=batch)
    return [stem_op(stem, h2, w2, 2), mp], [stem_op(fused, h4, w4, 4)], (h4, w4)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("case", [  # (H, W, batch, input, weights)
    (64, 128, 1, "u8", "plain"),        # pooled 16 x 32: whole 4 x 16 tiles
    (70, 134, 1, "u8", "plain"),        # pooled 18 x 34: one row and column past a tile; conv height 35 is odd: the last window's bottom row is outside
    (37, 53, 1, "u8", "plain"),
    (1, 1, 1, "u8", "plain"),
    (37, 53, 2, "u8", "plain"),         # image 1 of a batch
    (37, 53, 1, "f32", "plain"),        # AVL_IN_F32_CHW
    (37, 53, 1, "u8", "nonfinite"),     # a NaN weight row and an Inf one: fmaxf drops a NaN operand in the ReLU and in the pool alike
])
def test_pooled_stem_equals_stem_then_maxpool(case, precision, cuda_device):
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import pack_stem_mfma
    H, W, B, fmt, weights = case
    tdt = torch.bfloat16 if precision == "bf16" else torch.float16
    did = _did(precision)
    g = torch.Generator().manual_seed(H * 7 + W)
    if fmt == "u8":
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(cuda_device)
    else:
        img = torch.randn((B, 3, H, W), generator=g).to(cuda_device)
    w = torch.randn((64, 3, 7, 7), generator=g, dtype=torch.float64) * (2.0 / 147) ** 0.5
    if weights == "nonfinite":
        w[5, 1, 3, 3] = float("nan")
        w[9, 0, 2, 4] = float("inf")
    wd = pack_stem_mfma(w).to(tdt).to(cuda_device)
    bd = (torch.randn(64, generator=g) * 0.1).to(cuda_device)
    h2, w2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h4, w4 = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1
    rows = lambda n: (B * n + 255) // 256 * 256
    stem = torch.zeros((rows(h2 * w2), 64), dtype=tdt, device=cuda_device)
    ref = torch.full((rows(h4 * w4), 64), FILL, dtype=tdt, device=cuda_device)
    got = torch.full((rows(h4 * w4), 64), FILL, dtype=tdt, device=cuda_device)
    two, one, _ = _stem_ops(did, img, wd, bd, stem, ref, got, (H, W), B, in_format=int(fmt == "f32"))
    _run_plan(two)
    _run_plan(one)
    n = B * h4 * w4
    assert float(ref[:n].float().nan_to_num(0.0, 0.0, 0.0).abs().max()) > 0
    if weights == "nonfinite":
        assert bool(torch.isinf(ref[:n, 9].float()).any()) and not bool(torch.isnan(ref[:n].float()).any())
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), "%r %s: differs from stem -> max-pool" % (case, precision)
    assert bool((got[n:] == FILL).all())          # rows past the pooled image stay untouched


def test_pooled_stem_preprocesses_a_raw_frame(cuda_device):
    """the PRE loader (raw BGR frame, camera1's model, INTER_AREA by 2) under the pooled epilogue: 48 x 64 from a 96 x 128 frame"""
    import numpy as np
    import torch
    from vision_semantic_segmentation_amd.camera import camera_setup_1
    from vision_semantic_segmentation_amd.network import SegNet, random_state_dict
    st = random_state_dict(seed=0)
    cam = camera_setup_1().scaled(128 / 1920.0, 96 / 1440.0)
    frame = torch.from_numpy(np.random.default_rng(2).integers(0, 256, size=(96, 128, 3), dtype=np.uint8)).to(cuda_device)
    outs = {}
    for fuse in (True, False):
        net = SegNet(st, 48, 64, precision="f16", device=cuda_device, raw_frame=(96, 128), fuse_passes=fuse)
        assert net.op_names[0] == ("backbone.conv1+maxpool" if fuse else "backbone.conv1") and net.ops[0].in2
        net.set_camera(cam.K, cam.dist)
        net.image.copy_(frame)
        n = 1 if fuse else 2
        net.run_prefix(n)
        outs[fuse] = net.op_output(n - 1)
    assert outs[True].shape == (12 * 16, 64) and float(outs[True].abs().max()) > 0
    assert torch.equal(outs[True], outs[False])
