"""Exactly computable cases for the two fusions of the default "mixed" plan that keep a split intermediate in LDS, shared by
test_fused_mixed_operands_cpu.py (operand conditions, the dispatch claims and the teeth of the comparison, without a GPU) and
test_gpu_fused_mixed_exact.py (which runs the ops and compares every buffer for equality).

WHAT THE KERNELS COMPUTE (read from csrc/seg_dwpw.hip and csrc/seg_bottleneck.hip; the expected values mirror exactly this).

k_dwpw_x / k_dwpw_xs<CLS> (AVL_OP_DWPW, w_split = 3), per 64-wide K-step, fp32 throughout:
    depthwise   a = relu(b1 + sum_t w1[t] x_lo[t] + sum_t w1[t] x_hi[t]): ONE fmaf chain that starts from the bias, the lo plane's nine taps
                first (k_dwpw_x has no lo plane); w1, b1 are fp32 (pack_dw_f32); a tap outside the image reads 0
    tile split  a_h = f16(a), a_l = f16(a - a_h)
    pointwise   acc = b2 + sum_k Wh a_l + Wh a_h + Wl a_h      (Wl a_l is never formed); Wh | Wl = the [hi 64 | lo 64] halves of each K
                block of `weight`
    no out_f32  y = relu(acc), out = f16(y), out_lo = f16(y - out) where out_lo is set; columns with nbase + 16 > N are not written
    out_f32     y_h = f16(y), y_l = f16(y - y_h) in LDS; logit = bc + sum Wc_h y_l + Wc_l y_h + Wc_h y_h with in3 = [hi | lo][32][256];
                fp32 logits for cls < in3_c, label = the FIRST maximal index among them
k_dwpw<f16, 2> (w_split = 1): the depthwise stage of k_dwpw (tap pairs in f16, `a` as ONE f16 plane: _exact_operands.dwpw_case), then
    Wh a + Wl a.
k_bottleneck<CIN, DS, T1LO, XLO, OLO> (AVL_OP_BOTTLENECK of layer1):
    conv1  t1 = relu(b1 + sum W1h x_h + W1l x_h) kept as f16(t1), with T1LO (w_split = 1, in_c = 64) also f16(t1 - hi); zero outside the
           image; x_lo never enters conv1
    conv2  t2 = relu(b2 + sum W2h t1h + W2l t1h [+ W2h t1l]), always split hi + lo
    conv3  v = b3 + sum W3h t2h + W3l t2h + W3h t2l; DS: + sum Wdh x_h + Wdl x_h as extra K steps, otherwise + x_h, then + x_lo with XLO
           (two fp32 additions after the sum); out = f16(relu(v)), out_lo = f16(relu(v) - out) with OLO

OPERANDS.  DECOUPLED weights: the shipped packers derive lo from the same matrix as hi, lo is then below 2^-11 of hi and no exact sum
shows both.  The kernels multiply what they are passed, so Wh and Wl (W1h / W1l, ..., Wc_h / Wc_l) are INDEPENDENT matrices: `weight` of
DWPW is the hi slot of pack_split_rows(Wh, 2) with the hi slot of pack_split_rows(Wl, 2) moved into its lo slot (splice_rows), in3 is
stack([Wc_h, Wc_l]) directly, and each of pack_bottleneck's three outputs is spliced along its [hi, lo] axis from two calls
(splice_fragments).  The CPU test shows that both helpers, fed split_f16(w) of a Gaussian w, reproduce the shipped packer's bytes.
The LDS lo tiles (a_l, y_l, t1l, t2l) are remainders of in-kernel roundings and cannot be decoupled: they become visible because about a
quarter of the intermediate's channels carry a bias in 2048 .. 4000 (the depthwise result, t1 under T1LO, t2), where the value needs 12 or
13 bits and the remainder is a small multiple of the case's unit; the following stage's weights on those channels are sparse and within
+-1 so that every output stays below f16's 65504.  Without T1LO t1 stays an integer below 2048: its single plane is exact.  x_lo of
k_dwpw_xs and of the XLO residual is an independent plane of +-{1/4, 1/2, 1}, non-zero on most elements, NOT a remainder of x_hi.
Depthwise weights of the w_split = 3 cases: +-{1, 2}, and one channel per K-step carries the single weight 2049 or 4097 on its centre tap
(not f16 values: rounding the fp32 depthwise weights to f16 changes stored bytes); weights and biases differ per K-step.

EXACTNESS.  Every term of every stage is a multiple of 1/8 (x_lo and the depthwise result 1/4, lo weights 1/2), and sum|term| + |bias| +
|residual| stays below 2^24 / 8 at every stage, so fp32 accumulation -- the fmaf chain included -- is exact in any order; asserted per case
and stage on the operands' own sum of |x| |w|, together with float32 evaluation == float64 evaluation of every pass.

CONDITIONS asserted per case on the expected buffers (want_dw / want_bn): >= 20 % of the expected hi values are not representable before
rounding; exact ties round down to even and up to even in the output split and in an intermediate split; the in-kernel lo tile is non-zero
on >= 10 % of the intermediate's live elements; the output lo plane is non-zero on >= 10 % of the live elements.  Classifier cases (the
logits are fp32 and exact, the condition on hi values does not apply): with four classes or more rows 1 and 3 of Wc are identical and carry
the largest bias, >= 20 % of the pixels have two or more classes tied at the maximum and the first index is expected (one class cannot
tie); the rows past in3_c repeat row 1 with a larger bias (they would win if they took part), except in the all-negative case, where they
are zero and every real logit is negative.  The 1 x 1 bottleneck cases (one pixel: 128 values of t2, 256 outputs) cannot hold every kind
of tie: they assert exact splits, a rounded output and a non-empty t2 lo tile only; the shares and ties are asserted on all other shapes.

EXPECTED BUFFERS: built with a fill (7.0, -7.0 for logits, 99 for labels) and compared WHOLE: hi and lo plane, the rows past the last pixel,
the columns outside an out_ld > N slice, the lo plane of forms that do not write it, logits [rows][in3_c] and labels.  The visiting order
"hole" names one tile twice and another never: that tile keeps its fill, which shows that order[slot] is read."""
import collections
import functools

import torch
import torch.nn.functional as F

import _exact_operands as X
from _gconv_mixed_operands import ties

FILL, FILL_LOGIT, FILL_LABEL = 7.0, -7.0, 99
UNIT = 0.125
LIMIT = 2 ** 24
f16, f64 = torch.float16, torch.float64


def _up(n, m):
    return (n + m - 1) // m * m


def _pick(g, shape, values):
    t = torch.tensor(values, dtype=torch.float32)
    return t[torch.randint(0, len(values), tuple(shape), generator=g)]


def _scatter_rows(g, w, cols, count, values):
    """in every row of w: zero the columns `cols`, then `count` of them (chosen per row) get one of `values`"""
    w[:, cols] = 0
    if len(cols) == 0 or count == 0:
        return w
    count = min(count, len(cols))
    sel = torch.rand((w.shape[0], len(cols)), generator=g).argsort(dim=1)[:, :count]
    w[torch.arange(w.shape[0]).view(-1, 1), cols[sel]] = _pick(g, sel.shape, values)
    return w


def _round(v, how):
    """float64 -> f16: None = nearest even (what the kernels do), "truncate", "half_away" """
    if how == "truncate":
        return X.round_toward_zero(v.contiguous(), "f16")
    if how == "half_away":
        return X.round_half_away(v.contiguous(), "f16")
    return v.to(f16)


def _split(v, how=None):
    """(hi, lo) float64 of an exact float64 value: hi = f16(v) under rounding `how`, lo = f16(v - hi) (nearest even)"""
    hi = _round(v, how).double()
    return hi, (v - hi).to(f16).double()


def _exact_split(v, what):
    hi, lo = _split(v)
    assert bool(torch.isfinite(hi).all()), "%s overflows f16" % what
    assert torch.equal(hi + lo, v), "%s: hi + lo does not hold the exact value" % what
    return hi, lo


def _mm(a, w, check, what):
    """a [M][K] . w [N][K]^T in float64; check: the float32 evaluation gives the same"""
    y = a @ w.t()
    if check:
        assert torch.equal((a.float() @ w.float().t()).double(), y), "%s: the float32 and float64 host evaluations differ" % what
    return y


def _bound(mag, what):
    assert float(mag.max()) / UNIT < LIMIT, "%s: exactness bound %g units of 1/8 >= 2^24" % (what, float(mag.max()) / UNIT)


def _unit(v, what):
    assert torch.equal(torch.round(v / UNIT) * UNIT, v), "%s is not a multiple of 1/8" % what


def splice_rows(p_hi, p_lo):
    """two results of pack_split_rows(., 2) -- f16 [rows][K / 64][hi 64 | lo 64] -> the hi slot of the first with the hi slot of the second
    in the lo slot"""
    rows = p_hi.shape[0]
    out = p_hi.reshape(rows, -1, 2, 64).clone()
    out[:, :, 1] = p_lo.reshape(rows, -1, 2, 64)[:, :, 0]
    return out.reshape(rows, -1).contiguous()


def splice_fragments(p_hi, p_lo):
    """two flat outputs of pack_bottleneck (.. [hi, lo][lane 64][8]) -> the hi fragments of the first with the hi fragments of the second
    in the lo slot"""
    out = p_hi.reshape(-1, 2, 512).clone()
    out[:, 1] = p_lo.reshape(-1, 2, 512)[:, 0]
    return out.reshape(-1).contiguous()


def _big_bias(g, n, share_big, hi=5000):
    u = torch.rand(n, generator=g)
    pos = torch.randint(2048, hi, (n,), generator=g).float()
    neg = -torch.randint(2049, hi, (n,), generator=g).float()
    small = torch.randint(-40, 41, (n,), generator=g).float()
    return torch.where(u < share_big, pos, torch.where(u < share_big + 0.08, neg, small))


def _conditions(v, what, hi_share=True):
    """the conditions on an exact value that a kernel splits: -> (share of hi values that round, ties down, ties up, share with a lo part)"""
    hi, lo = _exact_split(v, what)
    share = float((hi != v).double().mean())
    down, up = ties(v, hi.to(f16))
    lo_share = float((lo != 0).double().mean())
    if hi_share:
        assert share >= 0.2, "%s: only %.1f %% of the hi values round" % (what, 100 * share)
    assert down > 0 and up > 0, "%s: exact ties rounding down %d, up %d" % (what, down, up)
    assert lo_share >= 0.1, "%s: the lo part is non-zero in only %.1f %%" % (what, 100 * lo_share)
    return share, down, up, lo_share


# ===================================================================================================================== DWPW
# kernel: "w2" = k_dwpw<f16, 2> | "x" = k_dwpw_x | "xs" = k_dwpw_xs<false> | "cls" = k_dwpw_xs<true>; layout: w_layout (1 = 8 x 16 blocks)
# order: "tile" = dwpw_tile_order | "block" = dwpw_block_order | "rev" = the tiles backwards | "hole" = tile 0 twice, the last tile never
# ncls: in3_c; slices: in_ld > K and out_ld > N (channel slices of wider filled buffers); olo: out_lo set; allneg: every real logit negative
DCase = collections.namedtuple("DCase", "kernel B H W K N dil pad layout order ncls slices olo allneg", defaults=(0, "tile", 0, False, True, False))
DW_KERNELS = {"w2": "k_dwpw<f16, 2>", "x": "k_dwpw_x", "xs": "k_dwpw_xs<false>", "cls": "k_dwpw_xs<true>"}


def dw_id(c):
    return "%s-b%d-%dx%d-k%d-n%d-d%d-p%d-%s-%s%s%s%s%s" % (c.kernel, c.B, c.H, c.W, c.K, c.N, c.dil, c.pad, "blocks" if c.layout else "rows", c.order,
                                                        "-cls%d" % c.ncls if c.ncls else "", "-slices" if c.slices else "", "" if c.olo or c.ncls else "-nolo",
                                                        "-allneg" if c.allneg else "")


DW_CASES = [DCase("w2", 1, h, w, k, n, d, p) for h, w, k, n, d, p, _ in X.DWPW_CASES] + [
    DCase("w2", 1, 9, 9, 64, 48, 2, 2, olo=False),
    # ---- k_dwpw_x
    DCase("x", 1, 12, 21, 64, 256, 1, 1),                      # one K-step: no pipeline
    DCase("x", 1, 12, 21, 128, 256, 2, 2),
    DCase("x", 1, 12, 21, 512, 256, 1, 1),                     # eight K-steps: the parameter ring wraps twice
    DCase("x", 1, 6, 11, 2048, 256, 24, 24),                   # almost every tap outside
    DCase("x", 1, 9, 15, 64, 512, 1, 1),                       # two N tiles
    DCase("x", 1, 37, 31, 64, 256, 1, 1),                      # 1147 pixels: nine tiles on sixteen slots
    DCase("x", 1, 12, 21, 128, 256, 1, 1, slices=True),
    DCase("x", 2, 12, 21, 128, 256, 2, 2),                     # 252 pixels per image
    DCase("x", 1, 12, 21, 128, 256, 1, 1, olo=False),
    DCase("x", 1, 37, 31, 64, 256, 1, 1, order="hole"),
    # ---- k_dwpw_xs<false>
    DCase("xs", 1, 14, 23, 64, 256, 1, 0),                     # the decoder's geometry, rows: a tile spans six image rows
    DCase("xs", 1, 21, 40, 128, 256, 1, 0, 1, "block"),        # 19 x 38 outputs: 3 x 3 blocks, ragged both ways
    DCase("xs", 1, 20, 15, 64, 64, 1, 0, 1, "block"),          # one block column, N = 64
    DCase("xs", 1, 19, 27, 128, 256, 12, 12),
    DCase("xs", 1, 16, 16, 64, 512, 1, 1, 1, "block"),         # two N tiles
    DCase("xs", 1, 14, 23, 320, 256, 1, 0),                    # five K-steps: the first ring wrap
    DCase("xs", 1, 21, 40, 512, 256, 1, 0, 1, "block"),
    DCase("xs", 2, 14, 23, 64, 256, 1, 0),
    DCase("xs", 2, 21, 40, 64, 256, 1, 0, 1, "block"),
    DCase("xs", 1, 37, 31, 64, 256, 1, 1, 0, "rev"),
    DCase("xs", 1, 21, 40, 64, 256, 1, 0, 1, "rev"),
    DCase("xs", 1, 21, 40, 64, 256, 1, 0, 1, "hole"),
    DCase("xs", 1, 14, 23, 128, 64, 1, 0, slices=True),
    DCase("xs", 1, 14, 23, 64, 256, 1, 0, olo=False),
    # ---- k_dwpw_xs<true>
    DCase("cls", 1, 14, 23, 64, 256, 1, 0, 1, "block", 19),
    DCase("cls", 1, 14, 23, 512, 256, 1, 0, 0, "tile", 19),
    DCase("cls", 1, 14, 23, 64, 256, 1, 0, 0, "tile", 1),
    DCase("cls", 1, 21, 40, 64, 256, 1, 0, 1, "block", 5, allneg=True),
    DCase("cls", 1, 14, 23, 64, 256, 1, 0, 0, "tile", 32),
    DCase("cls", 2, 21, 40, 64, 256, 1, 0, 1, "block", 19),
    DCase("cls", 1, 21, 40, 512, 256, 1, 0, 1, "rev", 32),
]


def dw_dispatch(w_split, in_lo, out_f32):
    """launch_dwpw's choice, restated (validate_dwpw refuses w_split 2, in_lo or w_layout 1 without w_split 3, out_f32 without in_lo)"""
    if w_split == 3 and out_f32:
        return "cls"
    if w_split == 3:
        return "xs" if in_lo else "x"
    return "w2" if w_split else "k_dwpw<f16 | bf16, 1>"


def dw_geometry(c):
    oh, ow = c.H + 2 * c.pad - 2 * c.dil, c.W + 2 * c.pad - 2 * c.dil
    m = oh * ow
    mtiles = ((ow + 15) // 16) * ((oh + 7) // 8) if c.layout else (m + 127) // 128
    return dict(oh=oh, ow=ow, m=m, rows=_up(c.B * m + 1, 256), rows_in=_up(c.B * c.H * c.W + 1, 256), mtiles=mtiles, nk=c.K // 64, np=_up(c.N, 256),
                in_ld=c.K + 64 if c.slices else c.K, in_off=32 if c.slices else 0, out_ld=c.N + 32 if c.slices else c.N, out_off=16 if c.slices else 0)


def dw_order(c):
    from vision_semantic_segmentation_amd.network import dwpw_block_order, dwpw_tile_order
    g = dw_geometry(c)
    if c.order == "block":
        return dwpw_block_order(g["oh"], g["ow"])
    if c.order == "tile":
        return dwpw_tile_order(g["oh"], g["ow"], c.dil)
    o = torch.arange(g["mtiles"] - 1, -1, -1, dtype=torch.int32)
    if c.order == "hole":
        o = torch.arange(g["mtiles"], dtype=torch.int32)
        o[-1] = 0
    return o


def dw_live_rows(c):
    """bool [B * M]: the output pixels that a visited tile covers"""
    g = dw_geometry(c)
    m, ow = g["m"], g["ow"]
    pix = torch.arange(m)
    tile = (pix // ow // 8) * ((ow + 15) // 16) + (pix % ow) // 16 if c.layout else pix // 128
    seen = torch.zeros(g["mtiles"], dtype=torch.bool)
    seen[dw_order(c).long()] = True
    return seen[tile].repeat(c.B)


@functools.lru_cache(maxsize=4)
def dw_operands(c):
    """the matrices of a case: xh (xl) [B][H][W][K], w1 [K][9], b1, Wh / Wl [Np][K] (rows past N hold values that must reach no output),
    b2 [Np], Wc_h / Wc_l [32][256], bc [32]; big = the channels whose depthwise result lies beyond 2048"""
    s = X._seed(c.B, c.H, c.W, c.K, c.N, c.dil, c.pad, len(c.kernel))
    g = torch.Generator().manual_seed(s)
    K, N = c.K, c.N
    np_ = _up(N, 256)
    o = {}
    if c.kernel == "w2":
        d = X.dwpw_case(c.H, c.W, K, N, c.dil, c.pad, "f16")
        o["xh"], o["xl"], o["w1"], o["b1"] = d["x"], None, d["Wd"].reshape(K, 9).clone(), d["b1"]
        o["big"] = torch.zeros(K, dtype=torch.bool)
        wh = X.ints(s + 3, np_, K)
        wh[:N] = d["W4"].view(N, K)
        o["Wh"], o["Wl"] = wh, _pick(g, (np_, K), [0, 0, 0.5, -0.5, 1, -1, 1.5, -1.5])
        b2 = torch.full((np_,), 12345.0)
        b2[:N] = X.bias_for(N, s + 4, "f16", True)
        o["b2"] = b2
        return o
    o["xh"] = X.ints(s, c.B * c.H * c.W, K).reshape(c.B, c.H, c.W, K)
    o["xl"] = _pick(g, (c.B, c.H, c.W, K), [0.25, -0.25, 0.5, -0.5, 1, -1, 0.25, 0]) if c.kernel != "x" else None
    w1 = _pick(g, (K, 9), [0, 0, 1, -1, 2, -2])
    step = torch.arange(K // 64)
    odd = step * 64 + (7 * step + 3) % 64                      # one channel per K-step whose only weight is no f16 value
    w1[odd] = 0
    w1[odd, 4] = torch.where(step % 2 == 0, 2049.0, 4097.0)
    big = torch.zeros(K, dtype=torch.bool)
    big[torch.randperm(K, generator=g)[:K // 4]] = True
    big[odd] = False
    b1 = torch.where(big, torch.randint(2048, 4000, (K,), generator=g).float(), torch.randint(-20, 21, (K,), generator=g).float())
    o["w1"], o["b1"], o["big"], o["odd"] = w1, b1, big, odd
    bigc = torch.nonzero(big).reshape(-1)
    wh = _scatter_rows(g, X.ints(s + 3, np_, K), bigc, 4, [1.0, -1.0])
    o["Wh"] = _scatter_rows(g, wh, odd, 1, [1.0, -1.0])
    wl = _scatter_rows(g, _pick(g, (np_, K), [0, 0, 0.5, -0.5, 1, -1, 1.5, -1.5]), bigc, 2, [0.5, -0.5, 1.0, -1.0])
    wl[:, odd] = 0
    o["Wl"] = wl
    b2 = torch.full((np_,), 12345.0)
    b2[:N] = _big_bias(g, N, 0.6)
    o["b2"] = b2
    if c.kernel == "cls":
        n = c.ncls
        wch = _pick(g, (32, 256), [0] * 14 + [1, -1])
        wcl = _pick(g, (32, 256), [0] * 14 + [0.5, -0.5])
        bc = torch.randint(-2000, 2001, (32,), generator=g).float()
        if n > 3:
            wch[3], wcl[3] = wch[1], wcl[1]
            bc[1] = bc[3] = 150000.0
        if c.allneg:
            bc[:n] -= 600000.0
            wch[n:], wcl[n:], bc[n:] = 0, 0, 0
        elif n > 3:
            wch[n:], wcl[n:], bc[n:] = wch[1], wcl[1], bc[1] + 1000.0
        o["Wc_h"], o["Wc_l"], o["bc"] = wch, wcl, bc
    return o


def _nchw(x):
    return x.permute(0, 3, 1, 2).double()


DW_MUTATIONS = ("drop_pass_0", "drop_pass_1", "drop_pass_2", "double_pass", "add_wl_al", "swap_slots", "drop_lo_taps", "tap8_missing",
                "clamped_halo", "stale_ring", "dw_f16", "mid_truncate", "mid_half_away", "out_truncate", "out_half_away", "drop_cls_yl",
                "last_index", "padding_classes", "row_past_m", "batch_halo")


def dw_applicable(c, mut):
    if mut in ("drop_pass_2", "add_wl_al", "mid_truncate", "mid_half_away", "dw_f16", "swap_slots"):
        return c.kernel != "w2"              # (k_dwpw<f16, 2> forms Wh a + Wl a on ONE plane: the sum does not know which slot is which)
    if mut == "drop_lo_taps":
        return c.kernel in ("xs", "cls")
    if mut == "stale_ring":
        return c.kernel != "w2" and c.K >= 320
    if mut in ("out_truncate", "out_half_away"):
        return c.kernel != "cls"
    if mut in ("drop_cls_yl", "last_index"):
        return c.kernel == "cls" and c.ncls > 3
    if mut == "padding_classes":
        return c.kernel == "cls" and c.ncls < 32
    if mut == "clamped_halo":
        return c.pad > 0
    if mut == "batch_halo":
        return c.B > 1 and c.pad == c.dil
    return True


def dw_depthwise(c, o, mut=None, check=False):
    """a = relu(b1 + the nine taps of both planes), float64 [B * M][K]"""
    K = c.K
    w1, b1 = o["w1"].double(), o["b1"].double()
    if mut == "tap8_missing":
        w1 = w1.clone()
        w1[:, 8] = 0
    if mut == "dw_f16":
        w1 = w1.to(f16).double()
    if mut == "stale_ring":                                    # the parameters of K-step s taken from step s - 4: the ring slot not refilled
        w1, b1 = w1.clone(), b1.clone()
        w1[256:], b1[256:] = o["w1"].double()[:K - 256], o["b1"].double()[:K - 256]
    planes = [o["xh"]] + ([o["xl"]] if o.get("xl") is not None and mut != "drop_lo_taps" else [])

    def conv(x, w, dtype=f64):
        xn = _nchw(x).to(dtype)
        pad = c.pad
        if mut == "batch_halo":                                # the images stacked: image n's halo reads its neighbours' rows
            xn = xn.permute(1, 0, 2, 3).reshape(1, K, c.B * c.H, c.W)
        if mut == "clamped_halo":
            xn, pad = F.pad(xn, (c.pad,) * 4, mode="replicate"), 0
        y = F.conv2d(xn, w.to(dtype).view(K, 1, 3, 3), None, padding=pad, dilation=c.dil, groups=K)
        if mut == "batch_halo":
            y = y.reshape(K, c.B, c.H, c.W).permute(1, 0, 2, 3)
        return y.permute(0, 2, 3, 1).reshape(-1, K)
    acc = sum(conv(x, w1) for x in planes)
    if check:
        for x in planes:
            assert torch.equal(conv(x, w1, torch.float32).double(), conv(x, w1)), "depthwise: the float32 and float64 host evaluations differ"
        _bound(sum(conv(x.abs(), w1.abs()) for x in planes) + b1.abs(), "depthwise")
    return torch.relu(acc + b1)


def dw_exact(c, o, mut=None, check=False):
    """-> dict(a, ah, al, y [, logits, labels]): the exact values of every stage (float64), optionally subtly wrong (DW_MUTATIONS)"""
    N, np_ = c.N, _up(c.N, 256)
    a = dw_depthwise(c, o, mut, check)
    if c.kernel == "w2":
        ah, al = a.to(f16).double(), torch.zeros_like(a)       # ONE f16 plane (exact on these operands: asserted)
        if check:
            assert torch.equal(a.to(f16).double(), a) and float(a.max()) < 256
    else:
        ah, al = _split(a, {"mid_truncate": "truncate", "mid_half_away": "half_away"}.get(mut))
        if check:
            _unit(a, "the depthwise result")
            _exact_split(a, "the depthwise result")
    Wh, Wl = o["Wh"][:N].double(), o["Wl"][:N].double()
    if mut == "swap_slots":
        Wh, Wl = Wl, Wh
    passes = ([(Wh, al)] if c.kernel != "w2" else []) + [(Wh, ah), (Wl, ah)]
    if mut is not None and mut.startswith("drop_pass_"):
        del passes[int(mut[-1])]
    elif mut == "double_pass":
        passes.append(passes[-1])
    elif mut == "add_wl_al":
        passes.append((Wl, al))
    b2 = o["b2"][:N].double()
    acc = b2 + sum(_mm(t, w, check, "pointwise") for w, t in passes)
    if check:
        _bound(sum(t.abs() @ w.abs().t() for w, t in passes) + b2.abs(), "pointwise")
        _unit(acc, "the pointwise sum")
    r = {"a": a, "ah": ah, "al": al, "y": torch.relu(acc)}
    if c.kernel == "cls":
        yh, yl = _split(r["y"])
        if check:
            _exact_split(r["y"], "the block's result")
        wch, wcl, bc = o["Wc_h"].double(), o["Wc_l"].double(), o["bc"].double()
        cp = ([] if mut == "drop_cls_yl" else [(wch, yl)]) + [(wcl, yh), (wch, yh)]
        lg = bc + sum(_mm(t, w, check, "classifier") for w, t in cp)
        if check:
            _bound(sum(t.abs() @ w.abs().t() for w, t in cp) + bc.abs(), "classifier")
            assert torch.equal(lg.float().double(), lg)
        n = 32 if mut == "padding_classes" else c.ncls
        top = lg[:, :n].max(dim=1, keepdim=True).values
        at = lg[:, :n] == top
        idx = torch.arange(n).view(1, -1).expand_as(at)
        r["labels"] = torch.where(at, idx, torch.full_like(idx, -1)).max(dim=1).values if mut == "last_index" else \
            torch.where(at, idx, torch.full_like(idx, 99)).min(dim=1).values
        r["logits"], r["tied"] = lg[:, :c.ncls], float((at.sum(dim=1) > 1).double().mean())
        assert mut is not None or (bool((r["labels"] >= 0).all()) and bool((r["labels"] < n).all()))
    return r


def dw_stored(c, r, mut=None):
    """every byte the op may touch, around its fill: {"out", "out_lo": f16 [rows][out_ld]} or {"logits": f32 [rows][ncls], "labels": uint8 [rows]}"""
    g = dw_geometry(c)
    rows, bm = g["rows"], c.B * g["m"]
    live = dw_live_rows(c)
    src = torch.arange(bm)
    if mut == "row_past_m":
        live, src = torch.cat([live, torch.tensor([True])]), torch.cat([src, torch.tensor([bm - 1])])
    dst = torch.nonzero(live).reshape(-1)
    src = src[live]
    if c.kernel == "cls":
        lg = torch.full((rows, c.ncls), FILL_LOGIT, dtype=torch.float32)
        lb = torch.full((rows,), FILL_LABEL, dtype=torch.uint8)
        lg[dst], lb[dst] = r["logits"].float()[src], r["labels"].to(torch.uint8)[src]
        return {"logits": lg, "labels": lb}
    hi = _round(r["y"], {"out_truncate": "truncate", "out_half_away": "half_away"}.get(mut))
    assert mut is not None or bool(torch.isfinite(hi).all()), "an expected output overflows f16"
    lo = (r["y"] - hi.double()).to(f16)
    out = torch.full((rows, g["out_ld"]), FILL, dtype=f16)
    out_lo = torch.full((rows, g["out_ld"]), FILL, dtype=f16)
    cols = slice(g["out_off"], g["out_off"] + c.N)
    out[dst, cols] = hi[src]
    if c.olo:
        out_lo[dst, cols] = lo[src]
    return {"out": out, "out_lo": out_lo}


def dw_evaluate(c, mut=None):
    return dw_stored(c, dw_exact(c, dw_operands(c), mut), mut)


@functools.lru_cache(maxsize=2)
def want_dw(c):
    """(exact stages, expected buffers); asserts every condition of the module docstring"""
    o = dw_operands(c)
    r = dw_exact(c, o, check=True)
    if c.kernel != "w2":
        a = r["a"]
        assert bool((o["w1"].to(f16).float() != o["w1"]).any()), "every depthwise weight is an f16 value"
        if c.kernel == "x":
            a = a[:, o["big"]]                                 # integers: only the channels beyond 2048 have a remainder; a quarter of the tile
            assert float(o["big"].double().mean()) >= 0.2
        r["mid"] = _conditions(a, "the depthwise result", hi_share=False)
        assert float((r["al"] != 0).double().mean()) >= 0.1, "the lo tile is non-zero on only %.1f %%" % (100 * float((r["al"] != 0).double().mean()))
    if c.kernel == "cls":
        _conditions(r["y"], "the block's result (y_h | y_l)")
        if c.ncls > 3:
            assert r["tied"] >= 0.2, "only %.1f %% of the pixels have tied maxima" % (100 * r["tied"])
            assert int((r["labels"] == 1).sum()) > 0 and int((r["labels"] == 3).sum()) == 0
        if c.allneg:
            assert bool((r["logits"] < 0).all())
    else:
        r["out"] = _conditions(r["y"], "the output")
    return r, dw_stored(c, r)


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k].view(torch.int16) if a[k].dtype == f16 else a[k], b[k].view(torch.int16) if b[k].dtype == f16 else b[k]) for k in a)


def dw_weight(o):
    """`weight` as the device reads it: f16 [Np][K / 64][Wh 64 | Wl 64], spliced from two calls of the shipped packer"""
    from vision_semantic_segmentation_amd.network import pack_split_rows
    return splice_rows(pack_split_rows(o["Wh"].double(), 2), pack_split_rows(o["Wl"].double(), 2))


def dw_device_inputs(c):
    """{"x": f16 [2][rows_in][in_ld] (plane 1 = in_lo; NaN in the rows past the last pixel and where unused, 5.0 in the columns outside the
    slice), "weight", "bias", "params": int32 depthwise parameters + visiting order [, "wc": f16 [2][32][256], "bc": f32 [32]]}"""
    from vision_semantic_segmentation_amd.network import pack_dw_f32, pack_dw_pairs
    o, g = dw_operands(c), dw_geometry(c)
    n_in = c.B * c.H * c.W
    x = torch.full((2, g["rows_in"], g["in_ld"]), float("nan"), dtype=f16)
    x[:, :n_in] = 5.0
    cols = slice(g["in_off"], g["in_off"] + c.K)
    x[0, :n_in, cols] = o["xh"].reshape(n_in, c.K).to(f16)
    if o["xl"] is not None:
        x[1, :n_in, cols] = o["xl"].reshape(n_in, c.K).to(f16)
    w1 = o["w1"].reshape(c.K, 1, 3, 3).double()
    dwp = pack_dw_pairs(w1, o["b1"].double(), f16) if c.kernel == "w2" else pack_dw_f32(w1, o["b1"].double())
    order = dw_order(c)
    assert order.numel() == g["mtiles"]
    d = {"x": x, "weight": dw_weight(o), "bias": o["b2"].clone(), "params": torch.cat([dwp, order])}
    if c.kernel == "cls":
        d["wc"], d["bc"] = torch.stack([o["Wc_h"], o["Wc_l"]]).to(f16).contiguous(), o["bc"].clone()
    return d


def make_dw_op(c, ptr):
    """the case's op; ptr: {"in", "in_lo", "weight", "bias", "params", "out", "out_lo", "wc", "bc", "logits", "labels"} -> address of element 0
    of each buffer (the slice offsets are added here)"""
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_DWPW, AvlSegOp
    g = dw_geometry(c)
    op = AvlSegOp()
    op.kind, op.dtype, op.batch = OP_DWPW, _lib.AVL_F16, c.B if c.B > 1 else 0
    op.in_, op.in2, op.weight, op.bias = ptr["in"] + 2 * g["in_off"], ptr["params"], ptr["weight"], ptr["bias"]
    op.w_split, op.w_layout = (1 if c.kernel == "w2" else 3), c.layout
    if c.kernel in ("xs", "cls"):
        op.in_lo = ptr["in_lo"] + 2 * g["in_off"]
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = c.H, c.W, c.K, g["in_ld"], g["rows_in"]
    op.out_h, op.out_w, op.out_c, op.out_rows = g["oh"], g["ow"], c.N, g["rows"]
    op.relu, op.w_rows, op.ksize, op.stride, op.pad, op.dil, op.groups = 1, g["np"], 3, 1, c.pad, c.dil, c.K
    if c.kernel == "cls":
        op.in2_lo, op.in3, op.in3_c = ptr["bc"], ptr["wc"], c.ncls
        op.out, op.out_mx, op.out_f32, op.out_ld = ptr["logits"], ptr["labels"], 1, c.ncls
    else:
        op.out, op.out_ld = ptr["out"] + 2 * g["out_off"], g["out_ld"]
        if c.olo:
            op.out_lo = ptr["out_lo"] + 2 * g["out_off"]
    return op


# =============================================================================================================== bottleneck
# k_bottleneck<CIN, DS, T1LO, XLO, OLO>: DS = (cin == 64); slices: in_ld > in_c and out_ld > 256
BCase = collections.namedtuple("BCase", "cin t1lo xlo olo B H W slices", defaults=(False,))
WIDTH, COUT, GROUPS = 128, 256, 32


def bn_id(c):
    return "cin%d-ds%d-t1lo%d-xlo%d-olo%d-b%d-%dx%d%s" % (c.cin, c.cin == 64, c.t1lo, c.xlo, c.olo, c.B, c.H, c.W, "-slices" if c.slices else "")


def bn_kernel(c):
    return "k_bottleneck<%d, %s, %s, %s, %s>" % (c.cin, *("true" if f else "false" for f in (c.cin == 64, c.t1lo, c.xlo, c.olo)))


def bn_dispatch(in_c, w_split, in_lo, out_lo):
    """launch_bottleneck's switch, restated: -> (CIN, DS, T1LO, XLO, OLO)"""
    variant = (4 + 2 * (1 if w_split else 0) if in_c == 64 else 2 * (1 if in_lo else 0)) + (1 if out_lo else 0)
    return [(256, False, False, False, False), (256, False, False, False, True), (256, False, False, True, False), (256, False, False, True, True),
            (64, True, False, False, False), (64, True, False, False, True), (64, True, True, False, False), (64, True, True, False, True)][variant]


BN_MANY = (270, 240)                                           # 34 x 15 = 510 tiles: two per workgroup on 256 CUs
BN_CASES = [
    BCase(64, True, False, True, 1, 8, 16), BCase(64, True, False, True, 1, 23, 45), BCase(64, True, False, True, 1, 3, 200),
    BCase(64, True, False, True, 2, 23, 45), BCase(64, True, False, True, 1, *BN_MANY),
    BCase(64, True, False, False, 1, 23, 45), BCase(64, True, False, False, 1, 70, 5),
    BCase(64, False, False, True, 1, 23, 45), BCase(64, False, False, True, 1, 23, 45, True),
    BCase(64, False, False, False, 1, 23, 45), BCase(64, False, False, False, 1, 1, 1),
    BCase(256, False, False, True, 1, 8, 16), BCase(256, False, False, True, 1, 23, 45),
    BCase(256, False, False, False, 1, 23, 45), BCase(256, False, False, False, 1, 70, 5),
    BCase(256, False, True, True, 1, 23, 45), BCase(256, False, True, True, 2, 23, 45), BCase(256, False, True, True, 1, 23, 45, True),
    BCase(256, False, True, True, 1, 1, 1), BCase(256, False, True, True, 1, *BN_MANY),
    BCase(256, False, True, False, 1, 70, 5), BCase(256, False, True, False, 1, 3, 200),
]


def bn_geometry(c, cus=256):
    m = c.H * c.W
    tiles = ((c.W + 15) // 16) * ((c.H + 7) // 8)
    grid = min(tiles, cus)
    return dict(m=m, rows=_up(c.B * m + 1, 256), tiles=tiles, tpw=-(-tiles // grid), in_ld=c.cin + 64 if c.slices else c.cin,
                in_off=32 if c.slices else 0, out_ld=COUT + 32 if c.slices else COUT, out_off=16 if c.slices else 0)


@functools.lru_cache(maxsize=2)
def bn_operands(cin, t1lo, B, H, W):
    s = X._seed(cin, t1lo, B, H, W, 99)
    g = torch.Generator().manual_seed(s)
    o = {"xh": X.ints(s, B * H * W, cin).reshape(B, H, W, cin), "xl": _pick(g, (B, H, W, cin), [0.25, -0.25, 0.5, -0.5, 1, -1, 0.25, 0])}
    bigg = torch.arange(GROUPS)[torch.arange(GROUPS) % 4 == 1]                    # eight groups: 32 of the 128 channels
    big2 = (bigg.view(-1, 1) * 4 + torch.arange(4)).reshape(-1)                  # the t2 channels with a bias beyond 2048
    big1 = bigg * 4                                                               # T1LO: the t1 channels with a bias beyond 2048 (one per big group)
    o["W1h"] = _pick(g, (WIDTH, cin), [0, 0, 0, 0, 0, 0, 1, -1])
    o["W1l"] = _pick(g, (WIDTH, cin), [0, 0, 0, 0, 0, 0, 0.5, -0.5] if t1lo else [0, 0, 0, 0, 0, 0, 1, -1])
    b1 = torch.randint(-10, 11, (WIDTH,), generator=g).float()
    if t1lo:
        b1[big1] = torch.randint(2048, 4000, (len(big1),), generator=g).float()
    w2h = _pick(g, (WIDTH, 4, 9), [0, 0, 0, 1, -1, 2, -2, 1, -1])
    w2l = _pick(g, (WIDTH, 4, 9), [0, 0, 0.5, -0.5, 1, -1])
    if t1lo:                                                                      # input channel 0 of a big group is a big t1 channel
        rows = big2
        w2h[rows, 0] = _scatter_rows(g, torch.zeros(len(rows), 9), torch.arange(9), 2, [1.0, -1.0])
        w2l[rows, 0] = _scatter_rows(g, torch.zeros(len(rows), 9), torch.arange(9), 1, [0.5, -0.5])
    b2 = torch.randint(-20, 21, (WIDTH,), generator=g).float()
    b2[big2] = torch.randint(2048, 4000, (len(big2),), generator=g).float()
    o["W2h"], o["W2l"], o["b1"], o["b2"] = w2h.reshape(WIDTH, 4, 3, 3), w2l.reshape(WIDTH, 4, 3, 3), b1, b2
    o["W3h"] = _scatter_rows(g, _pick(g, (COUT, WIDTH), [0, 0, 0, 1, -1, 1, -1, 2, -2]), big2, 3, [1.0, -1.0])
    o["W3l"] = _scatter_rows(g, _pick(g, (COUT, WIDTH), [0, 0, 0, 0.5, -0.5, 1, -1]), big2, 1, [0.5, -0.5])
    o["Wdh"], o["Wdl"] = X.ints(s + 5, COUT, cin), _pick(g, (COUT, cin), [0, 0, 0.5, -0.5, 1, -1])
    o["b3"] = _big_bias(g, COUT, 0.6)
    o["big1"], o["big2"] = big1, big2
    return o


def bn_ops_of(c):
    return bn_operands(c.cin, c.t1lo, c.B, c.H, c.W)


BN_MUTATIONS = ("c1_drop_lo", "c2_drop_lo", "c2_drop_t1l", "c3_drop_pass_0", "c3_drop_pass_1", "c3_drop_pass_2", "c3_double_pass", "c3_add_wl_tl",
                "swap_slots", "tap8_missing", "t1_not_zeroed", "t1_truncate", "t1_half_away", "t2_truncate", "t2_half_away", "out_truncate",
                "out_half_away", "drop_res_lo", "res_after_relu", "drop_downsample", "row_past_m", "batch_halo")


def bn_applicable(c, mut):
    if mut in ("c2_drop_t1l", "t1_truncate", "t1_half_away"):
        return bool(c.t1lo)
    if mut == "drop_res_lo":
        return bool(c.xlo)
    if mut == "res_after_relu":
        return c.cin == 256
    if mut == "drop_downsample":
        return c.cin == 64
    if mut == "batch_halo":
        return c.B > 1
    return True


def bn_exact(c, o, mut=None, check=False):
    """-> dict(t1, t2, v, y): the exact values of every stage (float64 [B * M][channels]), optionally subtly wrong (BN_MUTATIONS)"""
    B, H, W, cin = c.B, c.H, c.W, c.cin
    ds = cin == 64
    w = {k: o[k].double() for k in ("W1h", "W1l", "W2h", "W2l", "W3h", "W3l", "Wdh", "Wdl")}
    if mut == "swap_slots":
        w = {k[:-1] + ("l" if k[-1] == "h" else "h"): v for k, v in w.items()}
    if mut == "tap8_missing":
        for k in ("W2h", "W2l"):
            w[k] = w[k].clone()
            w[k][:, :, 2, 2] = 0
    x = o["xh"].reshape(-1, cin).double()
    xl = o["xl"].reshape(-1, cin).double()
    # ---- conv1
    p1 = [w["W1h"]] + ([] if mut == "c1_drop_lo" else [w["W1l"]])
    t1 = torch.relu(o["b1"].double() + sum(_mm(x, m, check, "conv1") for m in p1))
    if check:
        _bound(sum(x.abs() @ m.abs().t() for m in p1) + o["b1"].abs().double(), "conv1")
        _unit(t1, "t1")
    if c.t1lo:
        t1h, t1l = _split(t1, {"t1_truncate": "truncate", "t1_half_away": "half_away"}.get(mut))
        if check:
            _exact_split(t1, "t1")
    else:
        t1h, t1l = t1.to(f16).double(), None                   # ONE f16 plane (exact on these operands: asserted)
        if check:
            assert float(t1.max()) < 2048 and torch.equal(t1.to(f16).double(), t1), "t1 has no lo plane here: it must be an f16 value"

    def conv2(t, m, dtype=f64):
        tn = t.reshape(B, H, W, WIDTH).permute(0, 3, 1, 2).to(dtype)
        pad = 1
        if mut == "batch_halo":
            tn = tn.permute(1, 0, 2, 3).reshape(1, WIDTH, B * H, W)
        if mut == "t1_not_zeroed":                             # conv1 of the clamped pixel, which is what the X tile holds there
            tn, pad = F.pad(tn, (1, 1, 1, 1), mode="replicate"), 0
        y = F.conv2d(tn, m.to(dtype), None, padding=pad, groups=GROUPS)
        if mut == "batch_halo":
            y = y.reshape(WIDTH, B, H, W).permute(1, 0, 2, 3)
        return y.permute(0, 2, 3, 1).reshape(-1, WIDTH)
    p2 = [(t1h, w["W2h"])] + ([] if mut == "c2_drop_lo" else [(t1h, w["W2l"])]) + ([(t1l, w["W2h"])] if c.t1lo and mut != "c2_drop_t1l" else [])
    t2 = torch.relu(o["b2"].double() + sum(conv2(t, m) for t, m in p2))
    if check:
        for t, m in p2:
            assert torch.equal(conv2(t, m, torch.float32).double(), conv2(t, m)), "conv2: the float32 and float64 host evaluations differ"
        _bound(sum(conv2(t.abs(), m.abs()) for t, m in p2) + o["b2"].abs().double(), "conv2")
        _unit(t2, "t2")
        _exact_split(t2, "t2")
    t2h, t2l = _split(t2, {"t2_truncate": "truncate", "t2_half_away": "half_away"}.get(mut))
    # ---- conv3 (+ downsample | + identity)
    p3 = [(t2h, w["W3h"]), (t2h, w["W3l"]), (t2l, w["W3h"])]
    if mut is not None and mut.startswith("c3_drop_pass_"):
        del p3[int(mut[-1])]
    elif mut == "c3_double_pass":
        p3.append(p3[1])
    elif mut == "c3_add_wl_tl":
        p3.append((t2l, w["W3l"]))
    if ds and mut != "drop_downsample":
        p3 += [(x, w["Wdh"]), (x, w["Wdl"])]
    res = torch.zeros(()) if ds else x + (xl if c.xlo and mut != "drop_res_lo" else 0)
    v = o["b3"].double() + sum(_mm(t, m, check, "conv3") for t, m in p3)
    if check:
        _bound(sum(t.abs() @ m.abs().t() for t, m in p3) + o["b3"].abs().double() + res.abs().max(), "conv3")
        _unit(v + res, "the output")
    y = torch.relu(v) + res if mut == "res_after_relu" else torch.relu(v + res)
    return {"t1": t1, "t1l": t1l, "t2": t2, "t2l": t2l, "y": y}


def bn_stored(c, r, mut=None):
    """{"out", "out_lo": f16 [rows][out_ld]} around the fill"""
    g = bn_geometry(c)
    bm = c.B * g["m"]
    hi = _round(r["y"], {"out_truncate": "truncate", "out_half_away": "half_away"}.get(mut))
    assert mut is not None or bool(torch.isfinite(hi).all()), "an expected output overflows f16"
    lo = (r["y"] - hi.double()).to(f16)
    n = bm + (1 if mut == "row_past_m" else 0)
    src = torch.arange(n).clamp_max(bm - 1)
    out = torch.full((g["rows"], g["out_ld"]), FILL, dtype=f16)
    out_lo = torch.full((g["rows"], g["out_ld"]), FILL, dtype=f16)
    cols = slice(g["out_off"], g["out_off"] + COUT)
    out[:n, cols] = hi[src]
    if c.olo:
        out_lo[:n, cols] = lo[src]
    return {"out": out, "out_lo": out_lo}


def bn_evaluate(c, mut=None):
    return bn_stored(c, bn_exact(c, bn_ops_of(c), mut), mut)


@functools.lru_cache(maxsize=2)
def want_bn(c):
    o = bn_ops_of(c)
    r = bn_exact(c, o, check=True)
    small = c.H * c.W * c.B < 64                               # the 1 x 1 image: 256 outputs cannot hold every kind of tie
    if not small:
        if c.t1lo:
            r["mid1"] = _conditions(r["t1"][:, o["big1"]], "t1 on its channels beyond 2048", hi_share=False)
        r["mid2"] = _conditions(r["t2"][:, o["big2"]], "t2 on its channels beyond 2048", hi_share=False)
        assert float((r["t2l"] != 0).double().mean()) >= 0.1, "t2's lo tile is non-zero on only %.1f %%" % (100 * float((r["t2l"] != 0).double().mean()))
        r["out"] = _conditions(r["y"], "the output")
    else:
        _exact_split(r["y"], "the output")
        assert bool((r["y"] != r["y"].to(f16).double()).any()) and bool((r["t2l"] != 0).any())
    return r, bn_stored(c, r)


def bn_weights(c):
    """(p1, p2, p3): pack_bottleneck's three outputs with INDEPENDENT hi and lo fragments"""
    from vision_semantic_segmentation_amd.network import pack_bottleneck
    o = bn_ops_of(c)
    ds = c.cin == 64
    hi = pack_bottleneck(o["W1h"].double(), o["W2h"].double(), o["W3h"].double(), o["Wdh"].double() if ds else None, GROUPS)
    lo = pack_bottleneck(o["W1l"].double(), o["W2l"].double(), o["W3l"].double(), o["Wdl"].double() if ds else None, GROUPS)
    return tuple(splice_fragments(a, b) for a, b in zip(hi, lo))


def bn_device_inputs(c):
    """{"x": f16 [2][rows][in_ld] (plane 1 = in_lo; NaN past the last pixel and where unused, 5.0 outside the slice), "p1", "p2", "p3", "bias": b1 | b2 | b3}"""
    o, g = bn_ops_of(c), bn_geometry(c)
    bm = c.B * g["m"]
    x = torch.full((2, g["rows"], g["in_ld"]), float("nan"), dtype=f16)
    x[:, :bm] = 5.0
    cols = slice(g["in_off"], g["in_off"] + c.cin)
    x[0, :bm, cols] = o["xh"].reshape(bm, c.cin).to(f16)
    x[1, :bm, cols] = o["xl"].reshape(bm, c.cin).to(f16) if c.xlo else float("nan")
    p1, p2, p3 = bn_weights(c)
    return {"x": x, "p1": p1, "p2": p2, "p3": p3, "bias": torch.cat([o["b1"], o["b2"], o["b3"]])}


def make_bn_op(c, ptr):
    """ptr: {"in", "in_lo", "p1", "p2", "p3", "bias", "out", "out_lo"} -> address of element 0 of each buffer"""
    from vision_semantic_segmentation_amd import _lib
    from vision_semantic_segmentation_amd.network import OP_BOTTLENECK, AvlSegOp
    g = bn_geometry(c)
    op = AvlSegOp()
    op.kind, op.dtype, op.batch = OP_BOTTLENECK, _lib.AVL_F16, c.B if c.B > 1 else 0
    op.in_, op.out = ptr["in"] + 2 * g["in_off"], ptr["out"] + 2 * g["out_off"]
    op.weight, op.in2, op.in3, op.in3_c, op.bias = ptr["p1"], ptr["p2"], ptr["p3"], WIDTH, ptr["bias"]
    op.in_h, op.in_w, op.in_c, op.in_ld, op.in_rows = c.H, c.W, c.cin, g["in_ld"], g["rows"]
    op.out_h, op.out_w, op.out_c, op.out_ld, op.out_rows = c.H, c.W, COUT, g["out_ld"], g["rows"]
    op.ksize, op.stride, op.pad, op.dil, op.groups, op.relu = 3, 1, 1, 1, GROUPS, 1
    op.w_layout, op.w_split = int(c.cin == 64), int(c.t1lo)
    if c.xlo:
        op.in_lo = ptr["in_lo"] + 2 * g["in_off"]
    if c.olo:
        op.out_lo = ptr["out_lo"] + 2 * g["out_off"]
    return op
