"""What the max|ref|-relative bars of tests/test_gpu_mixed.py and tests/test_gpu_bottleneck.py let through, measured on the host (no GPU):

    python tools/fused_mutation_bars.py

Operands drawn as those tests draw them (Gaussian activations, Gaussian weights split into coupled hi + lo by split_f16), evaluated by
the host evaluators of tests/_fused_mixed_operands.py -- once as the kernels are documented to compute, once per deliberate mistake of its
mutation lists.  Printed per mistake: max|wrong - right| / max|right| of what the old test compares (hi + lo plane, or the logits) and
whether that is below the test's bar, i.e. whether a kernel with exactly this mistake and no other error would still pass.  (The exact
suite, tests/test_gpu_fused_mixed_exact.py, turns every one of them into a changed byte: tests/test_fused_mixed_operands_cpu.py.)
Mistakes that only move elements outside the compared region or only the labels are not listed: the old tests check those directly."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _fused_mixed_operands as M  # noqa: E402

TOL = 3e-6


def _split(w):
    from vision_semantic_segmentation_amd.network import split_f16
    hi, lo = split_f16(w.double())
    return hi.float(), lo.float()


def dw_gaussian(c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((c.B, c.H, c.W, c.K), generator=g, dtype=torch.float64)
    o = {"big": torch.zeros(c.K, dtype=torch.bool)}
    o["xh"], o["xl"] = _split(x)
    if c.kernel in ("w2", "x"):
        o["xl"] = None
    o["w1"] = (torch.randn((c.K, 9), generator=g) * 0.3).float()
    o["b1"] = torch.randn(c.K, generator=g) * 0.1
    o["Wh"], o["Wl"] = _split(torch.randn((c.N, c.K), generator=g, dtype=torch.float64) / c.K ** 0.5)
    o["b2"] = torch.randn(c.N, generator=g) * 0.1
    if c.kernel == "cls":
        wc = torch.zeros((32, 256), dtype=torch.float64)
        wc[:c.ncls] = torch.randn((c.ncls, 256), generator=g, dtype=torch.float64) / 16.0
        o["Wc_h"], o["Wc_l"] = _split(wc)
        o["bc"] = torch.zeros(32)
        o["bc"][:c.ncls] = torch.randn(c.ncls, generator=g) * 0.1
    return o


def dw_compared(c, r, mut):
    if c.kernel == "cls":
        return r["logits"]
    b = M.dw_stored(c, r, mut)
    n = c.B * M.dw_geometry(c)["m"]
    return b["out"][:n].double() + b["out_lo"][:n].double()


def bn_gaussian(c, seed):
    g = torch.Generator().manual_seed(seed)
    cin = c.cin
    o = {}
    o["xh"], o["xl"] = _split(torch.randn((c.B, c.H, c.W, cin), generator=g, dtype=torch.float64))
    for k, shape, s in (("W1", (128, cin), (2.0 / cin) ** 0.5), ("W2", (128, 4, 3, 3), (2.0 / 36) ** 0.5), ("W3", (256, 128), (1.0 / 128) ** 0.5),
                        ("Wd", (256, cin), (1.0 / cin) ** 0.5)):
        o[k + "h"], o[k + "l"] = _split(torch.randn(shape, generator=g, dtype=torch.float64) * s)
    b = torch.randn(512, generator=g) * 0.2
    o["b1"], o["b2"], o["b3"] = b[:128], b[128:256], b[256:]
    return o


def bn_compared(c, r, mut):
    b = M.bn_stored(c, r, mut)
    n = c.B * c.H * c.W
    return b["out"][:n].double() + (b["out_lo"][:n].double() if c.olo else 0)


SKIP = ("row_past_m", "last_index", "padding_classes")


def table(title, bar, c, o, exact, compared, mutations, applicable):
    right = compared(c, exact(c, o), None)
    scale = float(right.abs().max())
    print("%s   bar %.2e of max|ref|" % (title, bar))
    passed = []
    for mut in mutations:
        if mut in SKIP or not applicable(c, mut):
            continue
        err = float((compared(c, exact(c, o, mut), mut) - right).abs().max()) / scale
        print("    %-18s %.2e   %s" % (mut, err, "PASSES the bar" if err <= bar else "caught"))
        if err <= bar:
            passed.append(mut)
    return passed


def main():
    D, B = M.DCase, M.BCase
    dw = [("k_dwpw<f16, 2>      test_split_fused_depthwise_pointwise 37x53 K128 d12", 4 * 2 ** -11 / 128 ** 0.5, D("w2", 1, 37, 53, 128, 256, 12, 12)),
          ("k_dwpw_x            test_exact_fused_depthwise_pointwise 16x16 K256 N512 d1", 2 * TOL, D("x", 1, 16, 16, 256, 512, 1, 1)),
          ("k_dwpw_x            the same at K = 512, batch 2 (stale ring slot, neighbour image)", 2 * TOL, D("x", 2, 16, 16, 512, 256, 1, 1)),
          ("k_dwpw_xs<false>    ..._with_a_split_input 30x40 K1024 d12 p12", 2 * TOL, D("xs", 1, 30, 40, 1024, 256, 12, 12)),
          ("k_dwpw_xs<true>     ..._with_the_classifier_in_its_epilogue 20x31 K512 19 classes", 2 * TOL, D("cls", 1, 20, 31, 512, 256, 1, 0, 0, "tile", 19))]
    total = {}
    for title, bar, c in dw:
        total[title] = table(title, bar, c, dw_gaussian(c, 1), M.dw_exact, dw_compared, M.DW_MUTATIONS, M.dw_applicable)
    bn = [("k_bottleneck<64, DS, T1LO, -, OLO>   23x45", 3e-6, B(64, True, False, True, 2, 23, 45)),
          ("k_bottleneck<256, -, -, XLO, OLO>    23x45 (Gaussian t1: bar 3e-4)", 3e-4, B(256, False, True, True, 2, 23, 45)),
          ("k_bottleneck<256, -, -, -, ->        23x45 (single-plane output)", 1.5 * 2 ** -11, B(256, False, False, False, 1, 23, 45))]
    for title, bar, c in bn:
        total[title] = table(title, bar, c, bn_gaussian(c, 2), M.bn_exact, bn_compared, M.BN_MUTATIONS, M.bn_applicable)
    print("\nmistakes that pass their bar:")
    for title, muts in total.items():
        print("    %s: %s" % (title.split("   ")[0].strip(), ", ".join(muts) if muts else "none"))


if __name__ == "__main__":
    main()
