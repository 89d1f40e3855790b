"""Rule 9 of include/pt_hip.h, the guided upsampling onto supersampled planes, restated in numpy float32 twice on top
of tests/upsample_model.py, and seeded inputs for it.

model()    rule 8's whole-image model at the S-times size, then the sum over each S x S block as S * S strided adds
scalar()   rule 8's pixel-by-pixel model at the S-times size, then the sum pixel by pixel with np.float32 scalars

tests/test_upsample_resolve_rule.py holds the two against each other word for word; tests/test_gpu_upsample_resolve.py
holds the device against model().

`lo` = (color, plane0, plane1, plane2) of the low image, `ss` = (plane0, plane1, plane2) of the S-times frame.  Both
return (out, (count_wide, count_nearest)) with out of (ss height / S) x (ss width / S) x 4.
"""
import numpy as np

import upsample_model as um
from upsample_model import F, U, bits, same_words, PARAM_SETS, DEMODULATE, SAME_PRIMITIVE   # noqa: F401

FACTORS = (2, 3, 4)
FLAG_SETS = (0, DEMODULATE, SAME_PRIMITIVE, DEMODULATE | SAME_PRIMITIVE)
# (output width, output height, low width, low height): output sizes around the 32 x 8 tile and of several tiles; for
# each the low image equal to the output, half of it, and of a size that does not divide it (about two fifths)
OUTPUT_SIZES = ((1, 1), (31, 7), (32, 8), (33, 9), (48, 40))
SIZE_PAIRS = tuple(dict.fromkeys((W, H, w, h) for W, H in OUTPUT_SIZES
                                 for w, h in ((W, H), ((W + 1) // 2, (H + 1) // 2), (max(1, (2 * W + 4) // 5), max(1, (2 * H + 4) // 5)))))


def box_mean(img, S):
    """sum over j (outer), i (inner) of img[S Y + j, S X + i], begun at 0, then / (float)(S * S): rule 9's order."""
    img = np.ascontiguousarray(img, dtype=F)
    with np.errstate(all="ignore"):
        acc = np.zeros((img.shape[0] // S, img.shape[1] // S, 3), dtype=F)
        for j in range(S):
            for i in range(S):
                acc = (acc + img[j::S, i::S, :3]).astype(F)
        out = np.ones(acc.shape[:2] + (4,), dtype=F)
        out[..., :3] = (acc / F(S * S)).astype(F)
    return out


def model(lo, ss, S, sigma_plane, normal_power_log2, flags, stats=None):
    full, counts = um.model(lo, ss, sigma_plane, normal_power_log2, flags, stats)
    return box_mean(full, S), counts


def scalar(lo, ss, S, sigma_plane, normal_power_log2, flags):
    full, counts = um.scalar(lo, ss, sigma_plane, normal_power_log2, flags)
    Hs, Ws = full.shape[:2]
    H, W = Hs // S, Ws // S
    out = np.ones((H, W, 4), dtype=F)
    n = F(S * S)
    with np.errstate(all="ignore"):
        for Y in range(H):
            for X in range(W):
                for k in range(3):
                    s = F(0)
                    for j in range(S):
                        for i in range(S):
                            s = s + full[S * Y + j, S * X + i, k]
                    out[Y, X, k] = s / n
    return out, counts


def make_case(W, H, w, h, S, seed):
    """Seeded (lo, ss) of one scene: upsample_model.make_case with the S-times frame as its high image, so every case
    rule 8 distinguishes occurs among the sub-pixels (its stripes are six by five S-times pixels, so an output pixel's
    block often spans two ids)."""
    return um.make_case(S * W, S * H, w, h, seed)


def block_stats(ss0, S, wide_mask, nearest_mask):
    """How often the S x S blocks are of mixed ids, and hold a ring-2 or a nearest sub-pixel."""
    ids = bits(ss0[..., 3])
    H, W = ids.shape[0] // S, ids.shape[1] // S
    blocks = ids.reshape(H, S, W, S)
    mixed = (blocks != blocks[:, :1, :, :1]).any(axis=(1, 3))
    anyb = lambda m: m.reshape(H, S, W, S).any(axis=(1, 3))         # noqa: E731
    return {"mixed": int(mixed.sum()), "wide": int(anyb(wide_mask).sum()), "nearest": int(anyb(nearest_mask).sum()),
            "mixed_mask": mixed}
