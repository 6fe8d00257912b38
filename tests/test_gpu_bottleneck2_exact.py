"""AVL_OP_BOTTLENECK at 512 channels -- k_bottleneck_w256 (csrc/seg_bottleneck.hip), one identity Bottleneck of layer2 as one kernel with
the trunk in and out in the MX form -- ALONE through avl_seg_plan_* on exactly computable operands: the hi plane and both halves of the
output bundle, with the fill around them, are compared for equality with the exact result rounded once.

Why.  test_gpu_bottleneck_layer2.py sees this kernel at batch 1, with coupled hi / lo weights, through bars relative to max|ref| (3e-6
on the hi plane, 2^-13 on hi + lo) and a whole FP4 step on Q4(lo): profiles/bottleneck2_exact/mutation_bars.txt lists the deliberate
mistakes those bars let through.  The kernel streams X through a three-slab LDS-DMA ring with a hand-counted `s_waitcnt vmcnt(2)`,
prefetches across tiles, clears an overflow word in LDS once per tile and quantises two FP4 planes from a lane pair: a stale slab or a
word that is not cleared gives plausible numbers that only equality sees.

tests/_bottleneck2_operands.py builds the cases (its docstring states what the kernel computes and the operand design);
tests/test_bottleneck2_operands_cpu.py checks every condition, the dispatch claim and the teeth of the comparison without a GPU.  The
270 x 240 cases need more tiles than the device has CUs: the tests derive the tiles per workgroup from multi_processor_count and FAIL
below two (the X prefetch across tiles, load_w1(0) for the next tile, the reset of the overflow word).

No tolerance anywhere: bit equality."""
import pytest

import _bottleneck2_operands as M
from test_gpu_fused_mixed_exact import _compare

pytestmark = pytest.mark.gpu


def _run(c, d, cuda_device, repeat=1):
    """the case's op alone on the device inputs d -> [{"out", "out_mx"} on the host] per run"""
    import torch
    from test_gpu_ops import _run_plan
    from vision_semantic_segmentation_amd.network import mx_bundle_bytes
    g = M.geometry(c)
    d = {k: v.to(cuda_device) for k, v in d.items()}
    got = {"out": torch.full((g["rows"], M.COUT), M.FILL, dtype=torch.float16, device=cuda_device),
           "out_mx": torch.full((2, mx_bundle_bytes(g["rows"], M.COUT)), M.FILL_BYTE, dtype=torch.uint8, device=cuda_device)}
    ptr = {"in": d["x"].data_ptr(), "in_mx": d["in_mx"].data_ptr(), "p1": d["p1"].data_ptr(), "p2": d["p2"].data_ptr(), "p3": d["p3"].data_ptr(),
           "bias": d["bias"].data_ptr(), "out": got["out"].data_ptr(), "out_mx": got["out_mx"].data_ptr()}
    op = M.make_op(c, ptr)
    assert M.dispatch(op.in_c) == M.KERNEL, "%s no longer reaches %s" % (M.case_id(c), M.KERNEL)
    runs = []
    for _ in range(repeat):
        _run_plan([op])
        runs.append({k: v.cpu() for k, v in got.items()})
    return runs


def _planes(c, bufs):
    """the buffers cut into planes with one row per pixel row (together they are the whole buffers): the difference report then names rows"""
    rows = M.geometry(c)["rows"]
    p = {"out": bufs["out"]}
    for half, name in ((0, "hi"), (1, "lo")):
        q, s = M.unbundle(c, bufs["out_mx"], half)
        p["q4_" + name], p["scales_" + name] = q, s.permute(1, 0, 2).reshape(rows, -1)
    assert sum(t.numel() * t.element_size() for t in p.values()) == sum(t.numel() * t.element_size() for t in bufs.values())
    return p


def _tiles_per_workgroup(c, cuda_device):
    import torch
    g = M.geometry(c, torch.cuda.get_device_properties(cuda_device).multi_processor_count)
    assert g["tpw"] >= 2, "%s: %d tiles give %d per workgroup on this device: the case needs at least two" % (M.case_id(c), g["tiles"], g["tpw"])
    return g


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_layer2_bottleneck_exact(c, cuda_device):
    many = (c.H, c.W) == M.MANY
    if many:
        _tiles_per_workgroup(c, cuda_device)
    _, want = M.want(c)
    runs = _run(c, M.device_inputs(c), cuda_device, repeat=3 if many else 1)
    _compare(M.case_id(c), _planes(c, runs[0]), _planes(c, want), M.geometry(c)["bm"], c.W)
    assert M.same(runs[0], want)
    for n, r in enumerate(runs[1:]):
        assert M.same(r, runs[0]), "%s: launch %d differs from the first" % (M.case_id(c), n + 2)


def test_layer2_bottleneck_overflow_flags_exactly_the_tiles_that_hold_the_pixel(cuda_device):
    """One input pixel at the corner where four tiles meet drives one t1 channel beyond 65504.  A tile is flagged -- every live f16 of its hi
    plane has all exponent bits set -- if and only if its in-image 6 x 18 halo holds that pixel; every other tile, the next tile of a flagged
    tile's workgroup included, equals the no-overflow expectation bit for bit, and so do the rows past the last pixel."""
    import torch
    c = M.B2Case(1, *M.MANY)
    g = _tiles_per_workgroup(c, cuda_device)
    grid = min(g["tiles"], torch.cuda.get_device_properties(cuda_device).multi_processor_count)
    flagged = M.flagged_tiles(c)
    assert int(flagged.sum()) == 4
    for t in flagged[0].reshape(-1).nonzero().reshape(-1).tolist():
        assert t + grid < g["tiles"], "flagged tile %d is the last of its workgroup: nothing shows that the word is cleared" % t
    _, want = M.want(c)
    got = _run(c, M.overflow_inputs(c), cuda_device)[0]
    rows = M.flagged_rows(c)
    bits = got["out"].view(torch.int16).to(torch.int32) & 0xffff
    inf = (bits & 0x7c00) == 0x7c00
    assert bool(inf[rows].all()), "%d live f16 of the flagged tiles are finite" % int((~inf[rows]).sum())
    wrongly = inf[~rows].any(dim=1).nonzero().reshape(-1)
    assert wrongly.numel() == 0, "non-finite outputs outside the flagged tiles, rows %s (image y, x: %s)" % (
        wrongly[:8].tolist(), [(r // c.W, r % c.W) for r in wrongly[:8].tolist()])
    gp, wp = _planes(c, got), _planes(c, want)
    _compare(M.case_id(c) + "-overflow", {k: v[~rows] for k, v in gp.items()}, {k: v[~rows] for k, v in wp.items()}, int((~rows)[:g["bm"]].sum()), c.W)
    assert all(torch.equal(gp[k][g["bm"]:], wp[k][g["bm"]:]) for k in gp)
