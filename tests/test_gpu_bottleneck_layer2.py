"""AVL_OP_BOTTLENECK at 512 channels: one identity Bottleneck of ResNeXt-50 32x4d's layer2 (width 256, 32 groups of 8) as ONE kernel,
the trunk in and out in the MX form (hi f16 plane + bundle [Q4(hi) | scales | Q4(lo) | scales], the lo part only as FP4).

The op runs alone and is compared with a float64 evaluation of the block on the values its operands hold (weights hi + lo, the input's
hi plane for conv1, hi + the FP4 lo part for the residual), with the kernel's storage decisions mirrored: t1 is ONE f16 plane.  As in
test_gpu_bottleneck.py, "exact t1" operands (small-integer input hi parts and conv1 weights) make conv1 exact in fp32 and f16 alike, so
every intermediate keeps ~22 bits; then the output planes are checked one by one: the hi plane against float64, Q4(hi) byte for byte
against the host quantiser applied to that hi plane, and Q4(lo) against the FP4 grid around what hi left over."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CIN, WIDTH, COUT, G = 512, 256, 512, 32


def _split(x64):
    import torch
    hi = x64.to(torch.float16)
    lo = (x64 - hi.double()).to(torch.float16)
    return hi, lo


def _case(H, W, seed, cuda_device, exact_t1=True, repeat=1):
    import torch
    import torch.nn.functional as F
    from test_gpu_mixed import _bundle, _unbundle
    from test_gpu_ops import _from_rows, _nhwc_rows, _run_plan, _spatial_op
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import (AVL_MX_IN_LO, AVL_MX_OUT_LO, OP_BOTTLENECK, mx_bundle_bytes, mx_dequant_fp4,
                                                          mx_quant_fp4, pack_bottleneck)
    g = torch.Generator().manual_seed(seed)
    x64 = torch.randn((1, CIN, H, W), generator=g, dtype=torch.float64)
    w1 = torch.randn((WIDTH, CIN), generator=g, dtype=torch.float64) * (2.0 / CIN) ** 0.5
    w2 = torch.randn((WIDTH, WIDTH // G, 3, 3), generator=g, dtype=torch.float64) * (2.0 / (9 * WIDTH // G)) ** 0.5
    w3 = torch.randn((COUT, WIDTH), generator=g, dtype=torch.float64) * (1.0 / WIDTH) ** 0.5
    b = torch.randn(2 * WIDTH + COUT, generator=g) * 0.2
    if exact_t1:         # x hi = +-1, +-2 (the noise goes to the lo part), conv1 weights in {-1, 0, 1}, integer bias: |conv1| <= 2 cin + 3 < 2048
        x64 = (torch.randint(1, 3, x64.shape, generator=g) * (torch.randint(0, 2, x64.shape, generator=g) * 2 - 1)).double() + x64 * 1e-4
        w1 = torch.randint(-1, 2, w1.shape, generator=g).double() * (torch.rand(w1.shape, generator=g) < 0.25)
        b[:WIDTH] = torch.randint(-3, 4, (WIDTH,), generator=g).float()
        w2 = w2 * 0.1
    xh, xl = _split(x64)
    xh_rows = _nhwc_rows(xh)
    rows = xh_rows.shape[0]
    xin = _bundle(xh_rows.double()[:H * W], _nhwc_rows(xl).double()[:H * W], rows)
    xl_fp4 = _unbundle(xin, rows, CIN, 1)[2][:H * W]                       # the lo part as the kernel reads it

    def q(w):            # the value the kernel's hi + lo pair holds
        hi, lo = _split(w)
        return hi.double() + lo.double()

    t1 = F.relu(F.conv2d(xh.double(), q(w1).reshape(WIDTH, CIN, 1, 1), b[:WIDTH].double())).to(torch.float16).double()
    t2 = F.relu(F.conv2d(t1, q(w2), b[WIDTH:2 * WIDTH].double(), padding=1, groups=G))
    y = F.conv2d(t2, q(w3).reshape(COUT, WIDTH, 1, 1), b[2 * WIDTH:].double())
    y = y + xh.double() + xl_fp4.reshape(H, W, CIN).permute(2, 0, 1).unsqueeze(0)
    ref = F.relu(y)

    src = xh_rows.to(cuda_device)
    xin_d = xin.to(cuda_device)
    dst = torch.full((rows, COUT), 7.0, dtype=torch.float16, device=cuda_device)
    out_mx = torch.full((2 * mx_bundle_bytes(rows, COUT),), 0xA5, dtype=torch.uint8, device=cuda_device)
    p1, p2, p3 = (t.to(cuda_device) for t in pack_bottleneck(w1, w2, w3, None, G))
    bd = b.to(cuda_device)
    op = _spatial_op(OP_BOTTLENECK, _lib.AVL_F16, src, (H, W), CIN, dst, (H, W), COUT, weight=p1.data_ptr(), in2=p2.data_ptr(),
                     in3=p3.data_ptr(), in3_c=WIDTH, bias=bd.data_ptr(), ksize=3, stride=1, pad=1, dil=1, groups=G, relu=1, w_layout=0,
                     w_split=0, in_mx=xin_d.data_ptr(), out_mx=out_mx.data_ptr(), mx_flags=AVL_MX_IN_LO | AVL_MX_OUT_LO)
    _run_plan([op])
    hi = dst.cpu()
    bundle = out_mx.cpu()
    for _ in range(repeat - 1):          # repeated launches agree bit for bit (race screen)
        _run_plan([op])
        assert torch.equal(dst.cpu(), hi) and torch.equal(out_mx.cpu(), bundle)

    got = _from_rows(hi.double(), H, W, COUT)
    scale = float(ref.abs().max())
    # hi plane: float64 within an f16 rounding of the result (exact t1: ~22 bits before that rounding)
    bar = 3e-6 if exact_t1 else 3e-4
    err_hi = ((got - ref).abs() - 2 ** -11 * ref.abs()).clamp_min(0).max().item() / scale
    assert err_hi <= bar, "layer2 block %dx%d: hi plane %.3e (bar %.1e)" % (H, W, err_hi, bar)
    assert torch.all(hi[H * W:] == 7.0)
    # Q4(hi): the host quantiser's bytes of the hi plane the kernel wrote, rows past H * W untouched
    qh, sh, _ = _unbundle(bundle, rows, COUT, 0)
    eq, es = mx_quant_fp4(hi[:H * W].double())
    assert torch.equal(qh[:H * W], eq) and torch.equal(sh[:, :H * W], es)
    assert torch.all(qh[H * W:] == 0xA5) and torch.all(sh[:, H * W:] == 0xA5)
    # Q4(lo): the FP4 quantisation of what the hi plane left over (scale of each 32-block from its largest element)
    ql, sl, lo_deq = _unbundle(bundle, rows, COUT, 1)
    assert torch.all(ql[H * W:] == 0xA5) and torch.all(sl[:, H * W:] == 0xA5)
    lo_ref = ref[0].permute(1, 2, 0).reshape(H * W, COUT) - hi[:H * W].double()
    amax = lo_ref.reshape(H * W, COUT // 32, 32).abs().amax(dim=2, keepdim=True).expand(-1, -1, 32).reshape(H * W, COUT)
    err_lo = ((lo_deq[:H * W] - lo_ref).abs() - 0.25 * amax).clamp_min(0).max().item() / scale
    if exact_t1:
        assert err_lo <= 3e-6, "layer2 block %dx%d: FP4 lo part %.3e" % (H, W, err_lo)
    tot = (got + lo_deq[:H * W].reshape(H, W, COUT).permute(2, 0, 1).unsqueeze(0) - ref).abs().max().item() / scale
    assert tot <= (2 ** -13 if exact_t1 else 3e-4), "layer2 block %dx%d: hi + lo %.3e" % (H, W, tot)
    return err_hi, tot


@pytest.mark.parametrize("hw", [(4, 16), (37, 53), (5, 17), (1, 1), (135, 240)])
def test_layer2_block_exact_t1(hw, cuda_device):
    _case(hw[0], hw[1], hw[0] * 131 + hw[1], cuda_device)


@pytest.mark.parametrize("hw", [(37, 53), (135, 240)])
def test_layer2_block_gaussian(hw, cuda_device):
    """Gaussian operands: conv1 results close to an f16 rounding boundary may round the other way than float64's (t1 is one f16 plane)"""
    _case(hw[0], hw[1], 7 + hw[0], cuda_device, exact_t1=False)


def test_layer2_block_walks_several_tiles_per_workgroup(cuda_device):
    """1080p's 135 x 240 = 34 x 15 = 510 tiles and 270 x 240 = 1020: two and four tiles per workgroup (the X ring's prefetch across
    tiles); repeated launches agree bit for bit"""
    _case(270, 240, 11, cuda_device, repeat=3)
