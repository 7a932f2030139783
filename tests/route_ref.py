"""The conv dispatch restated in Python, for tests/test_conv_route_cpu.py: which packings a layer holds and which kernel, mode, tile and
layouts every launch of the encoder takes.  Written from the launch sequences as they stood before the library had a routing function
(the if-chain of run_conv, run_dual, the block walk of encoder_chunk, the use_* predicates and the packing conditions of hpe_finalize),
not from that function: the order of the tests below is the order those pieces ran in, with the caller / callee split kept
(`chunk_launches` decides the layouts and passes flags, `run_conv` obeys them).  Pure Python on the layer table, no library."""
import os

from hpe_amd.resnet_spec import CONV_SPECS

KERNELS = ("f32", "f32s", "bf16", "bf16_p8", "halo3", "wino", "wino_fused", "wino4", "wino4_fused")
OPT_IN = {"bf16_p8": "bf16_p8", "wino4_fused": "wino4_fused"}  # kernel -> the plan option that reaches it (off by default)
DENSE, STRIDED, CONV3, STEM, DUAL = 0, 1, 2, 3, 4
T128x128, T128x64, T64x64, T64x128, T128x128_W8, T128x64_W8, T256x128_W8, TP8 = range(8)
PACK_BITS = {"w_split": 1, "wino_u": 2, "wino4_u": 3, "stem_w": 4, "w_dual": 7, "w_dual_split": 8}  # HPE_PACK_* of include/hpe.h

# ---- the option table: name -> ((default fp32, bf16), (mask fp32, bf16)); None = every bit
OPTIONS = {
    "dual_gemm": ((1, 1), (None, None)), "wino_min_c": ((128, 128), (None, None)), "wino_min_items": ((128, 128), (None, None)),
    "wino_fused": ((1, 1), (None, None)), "wino_fused_min_hw": ((28, 28), (None, None)), "wino_f4": ((7, 7), (None, None)),
    "wino4_fused": ((0, 0), (12, 12)), "bf16_p8": ((0, 0), (None, None)), "chain_fuse": ((8, 7), (8, 23)), "halo3": ((15, 15), (0, 15)),
    "f32_split": ((14, 14), (15, 0)),
    # environment only: the tests run with none of them set
    "f32s_min_tiles": ((128, 128), (None, None)), "concurrent_tiles": ((0, 0), (None, None)), "bf16_w8_min_tiles": ((128, 128), (None, None)),
    "wide128_min_tiles": ((384, 384), (None, None)), "force_wide": ((-1, -1), (None, None)), "wino4_min_items": ((64, 64), (None, None)),
}
BF16_128_MIN_TILES, BF16_P8_MIN_N, BF16_P8_MIN_K, EXPAND_SMALL_GRID = 192, 256, 512, 128
F32S_EXPAND_MIN_K = 256
F32S_TILES = {T128x128: (128, 128), T128x128_W8: (128, 128), T256x128_W8: (256, 128)}


def resolve_plan(bf16, **opts):
    assert not [k for k in os.environ if k.startswith("HPE_")], "the restatement knows no environment"
    pl = {}
    for k, (dflt, mask) in OPTIONS.items():
        v = opts[k] if opts.get(k, -1) >= 0 else dflt[bf16]
        pl[k] = v if mask[bf16] is None else v & mask[bf16]
    unknown = set(opts) - set(OPTIONS)
    assert not unknown, unknown
    pl["wino_fused"] = int(bool(pl["wino_fused"]) and pl["wino_min_c"] > 0)
    if pl["wino_min_c"] <= 0:
        pl["wino_f4"] = pl["wino4_fused"] = 0
    return pl


def stage_bit(hout):
    return 1 if hout >= 56 else 2 if hout >= 28 else 4 if hout >= 14 else 8


def f4_bit(hin):
    return 1 if hin <= 7 else 2 if hin <= 14 else 4 if hin <= 28 else 8


def cdiv(a, b):
    return (a + b - 1) // b


def blocks():
    """(stage, first, last, i2a, i2b, i2c, i1) of the 16 bottleneck blocks, layers in the order [2a, 2b, 2c, (1)]"""
    out, i = [], 1
    for st, n in enumerate((3, 4, 6, 3)):
        for b in range(n):
            first = b == 0
            out.append((st, first, b == n - 1, i, i + 1, i + 2, i + 3 if first else -1))
            i += 4 if first else 3
    assert i == len(CONV_SPECS)
    return out


BLOCKS = blocks()


# ---- what hpe_finalize packs (pack_conv_weights, pack_dual_weights)
def packs(pl, bf16, idx):
    s = CONV_SPECS[idx]
    slab = 64 if bf16 else 32
    have = set()
    if idx == 0:
        have.add("stem_w")
    if not bf16:
        if idx != 0 and s.kh == 1 and pl["f32_split"] & stage_bit(s.hout):
            have.add("w_split")
        wino_geo = s.kh == 3 and s.stride == 1 and s.cin % 32 == 0 and s.cout % 64 == 0
        if pl["wino_min_c"] > 0 and wino_geo and (s.cin >= pl["wino_min_c"] or (pl["wino_fused"] and s.hin >= pl["wino_fused_min_hw"])):
            have.add("wino_u")
        if wino_geo and (pl["wino_f4"] | pl["wino4_fused"]) & f4_bit(s.hin):
            have.add("wino4_u")
    for (_, first, _, _, _, i2c, i1) in BLOCKS:
        if pl["dual_gemm"] and first and i2c == idx and s.cin % slab == 0 and CONV_SPECS[i1].cin % slab == 0:
            have.add("w_dual")
            if not bf16 and pl["f32_split"] & stage_bit(s.hout):
                have.add("w_dual_split")
    return have


def pack_mask(have):
    return sum(1 << PACK_BITS[n] for n in have)


def k_pad(idx, bf16):
    s = CONV_SPECS[idx]
    slab = 64 if bf16 else 32
    return cdiv(7 * 32 if idx == 0 else s.kh * s.kw * s.cin, slab) * slab


# ---- work items of the Winograd launches and the geometry the special kernels support
def wino4_items(B, H, N):
    return cdiv(B * cdiv(H, 4) * cdiv(H, 4), 32) * (N // 32)


def wino4_fused_items(B, H, N):
    if H not in (56, 28):
        return 0
    TW = H // 4
    if TW > 32:
        return 0
    R = 32 // TW
    while R > 1 and R * 6 * (H + 2) > 768:
        R -= 1
    if R * 6 * (H + 2) > 768:
        return 0
    R = min(R, (H // 4) * B)
    if R < 1:
        return 0
    return cdiv(B * (H // 4), R) * (N // 64)


def wino_fused_items(B, H, N):
    TW = H // 2
    if H & 1 or TW > 64 or TW < 1:
        return 0
    R = min(64 // TW, 960 // (16 * (TW + 1)))
    if R < 1:
        return 0
    return cdiv(B * TW, R) * (N // 64)


def halo3_supported(HW, cin, N):
    return (HW, cin, N) in ((56, 64, 64), (28, 128, 128), (14, 256, 256), (7, 512, 512))


def chain_bf16_supported(C, C4, CP, C2):
    if C4 != 4 * C or CP != C:
        return False
    return C in (64, 128, 256) if C2 == 0 else (C == 64 and C2 == 64)


def chain_f32_supported(C, C4, CP):
    return (C, C4, CP) == (64, 256, 64)


# ---- the predicates
def use_wino4(pl, bf16, have, idx, B):
    s = CONV_SPECS[idx]
    return (not bf16 and "wino4_u" in have and s.kh == 3 and s.stride == 1 and bool(pl["wino_f4"] & f4_bit(s.hin))
            and wino4_items(B, s.hin, s.cout) >= min(pl["wino_min_items"], pl["wino4_min_items"]))


def use_wino4_fused(pl, bf16, have, idx, B):
    s = CONV_SPECS[idx]
    return (not bf16 and "wino4_u" in have and s.kh == 3 and s.stride == 1 and bool(pl["wino4_fused"] & f4_bit(s.hin))
            and wino4_fused_items(B, s.hin, s.cout) >= min(pl["wino_min_items"], pl["wino4_min_items"]))


def use_wino_fused(pl, bf16, have, idx, B):
    s = CONV_SPECS[idx]
    if use_wino4_fused(pl, bf16, have, idx, B) or use_wino4(pl, bf16, have, idx, B):
        return False
    return (bool(pl["wino_fused"]) and not bf16 and "wino_u" in have and s.kh == 3 and s.stride == 1 and s.hin >= pl["wino_fused_min_hw"]
            and wino_fused_items(B, s.hin, s.cout) >= pl["wino_min_items"])


def use_chain(pl, bf16, blk):
    stg, first, last, _, _, i2c, _ = blk
    if last:
        return False
    s2 = CONV_SPECS[i2c]
    if not bf16:
        if first or stg != 0 or not pl["chain_fuse"] & 8:
            return False
        sn = CONV_SPECS[i2c + 1]
        return sn.kh == 1 and sn.stride == 1 and sn.cin == s2.cout and chain_f32_supported(s2.cin, s2.cout, sn.cout)
    if first:
        s1, sn = CONV_SPECS[i2c + 1], CONV_SPECS[i2c + 2]
        return (stg == 0 and bool(pl["chain_fuse"] & 4) and "w_dual" in packs(pl, bf16, i2c) and s1.stride == 1 and s1.hin == s2.hin and sn.kh == 1
                and sn.stride == 1 and sn.cin == s2.cout and chain_bf16_supported(s2.cin, s2.cout, sn.cout, s1.cin))
    bit = {0: 1, 1: 2, 2: 16}.get(stg, 0)
    if not pl["chain_fuse"] & bit:
        return False
    sn = CONV_SPECS[i2c + 1]
    return sn.kh == 1 and sn.stride == 1 and sn.cin == s2.cout and chain_bf16_supported(s2.cin, s2.cout, sn.cout, 0)


# ---- the tile rules
def pick_f32s(pl, split, M, N, K, expand):
    if not split or N <= 64:
        return -1
    if expand and K < F32S_EXPAND_MIN_K:
        return -1
    tile = T128x128_W8 if expand else T128x128
    bm, bn = F32S_TILES[tile]
    return tile if cdiv(M, bm) * cdiv(N, bn) >= pl["f32s_min_tiles"] else -1


def pick_tile(pl, M, N, K, expand, concurrent):
    wide = N > 64
    if wide and expand:
        return T64x64 if cdiv(M, 128) * cdiv(N, 64) < EXPAND_SMALL_GRID else T128x64_W8
    if wide and pl["force_wide"] >= 0:
        return pl["force_wide"]
    if not wide:
        return T128x64
    if K <= 128 and M >= 150000:
        return T128x64_W8
    if (concurrent or pl["concurrent_tiles"]) and pl["wide128_min_tiles"] > 0 and cdiv(M, 128) * cdiv(N, 128) >= pl["wide128_min_tiles"]:
        return T128x128
    if M >= 150000:
        return T64x128
    return T64x64


def pick_bf16(pl, M, N, K, expand, concurrent, mode):
    if pl["bf16_p8"] and N >= BF16_P8_MIN_N and N % 256 == 0 and K >= BF16_P8_MIN_K and not expand:
        bit = (1 if N == 256 else 2) if mode == CONV3 else ((8 if N >= 2048 else 16) if mode == DUAL else 4)
        if pl["bf16_p8"] & bit:
            return TP8
    if N <= 64:
        return T128x64
    t128 = cdiv(M, 128) * cdiv(N, 128)
    tile = T128x128 if t128 >= (BF16_128_MIN_TILES if (concurrent or pl["concurrent_tiles"]) else 512) else T64x128
    if expand:
        tile = T128x64_W8
    elif 8192 <= M <= 16384 and K >= 1024 and N >= 256:
        tile = T256x128_W8
    if pl["bf16_w8_min_tiles"] > 0 and t128 >= pl["bf16_w8_min_tiles"]:
        tile = T128x128_W8
    return tile


def gemm_kernel(pl, bf16, mode, M, N, K, expand, split, concurrent):
    """(kernel, tile) of the tail all GEMM launches share"""
    if bf16:
        tile = pick_bf16(pl, M, N, K, expand, concurrent, mode)
        return ("bf16_p8" if tile == TP8 else "bf16"), tile
    f32s = pick_f32s(pl, split, M, N, K, expand)
    if f32s >= 0:
        return "f32s", f32s
    return "f32", pick_tile(pl, M, N, K, expand, concurrent)


# ---- the launches
def run_conv(pl, bf16, idx, B, res, wino_v, in_slab8=False, out_slab8=False, concurrent=False):
    """the if-chain of one layer's launch -> dict(kernel, mode, tile, in_slab8, out_slab8); in_slab8 / out_slab8 are the caller's flags"""
    s = CONV_SPECS[idx]
    have = packs(pl, bf16, idx)
    mode = STEM if idx == 0 else CONV3 if s.kh == 3 else DENSE if s.stride == 1 else STRIDED
    out = dict(mode=mode, tile=-1, in_slab8=in_slab8, out_slab8=False)
    if in_slab8 and use_wino4_fused(pl, bf16, have, idx, B):
        return dict(out, kernel="wino4_fused")
    if in_slab8:
        return dict(out, kernel="wino_fused")
    if wino_v and not res and use_wino4(pl, bf16, have, idx, B):
        return dict(out, kernel="wino4")
    th = (s.hin + 1) // 2
    if "wino_u" in have and wino_v and not res and s.cin >= pl["wino_min_c"] and cdiv(B * th * th, 64) * (s.cout // 64) >= pl["wino_min_items"]:
        return dict(out, kernel="wino")
    M, N, K = B * s.hout * s.hout, s.cout, k_pad(idx, bf16)
    if bf16 and mode == CONV3 and not res and s.stride == 1 and pl["halo3"] & f4_bit(s.hin) and halo3_supported(s.hin, s.cin, s.cout) and K >= 9 * s.cin:
        return dict(out, kernel="halo3")
    expand = mode == DENSE and res and s.cout == 4 * s.cin
    split = "w_split" in have and mode in (DENSE, STRIDED)
    kernel, tile = gemm_kernel(pl, bf16, mode, M, N, K, expand, split, concurrent)
    return dict(out, kernel=kernel, tile=tile, out_slab8=out_slab8)


def debug_conv(pl, bf16, idx, B, res, workspace=True):
    """a layer on NHWC input, alone on the device (hpe_debug_conv, the training forward); workspace: the context has a V workspace"""
    have = packs(pl, bf16, idx)
    if not bf16 and not res and (use_wino_fused(pl, bf16, have, idx, B) or use_wino4_fused(pl, bf16, have, idx, B)):
        return run_conv(pl, bf16, idx, B, False, False, in_slab8=True)
    return run_conv(pl, bf16, idx, B, res, workspace and not bf16)


def chunk_launches(pl, bf16, B, concurrent, workspace):
    """the block walk of one batch chunk -> {layer index: launch dict}; a branch2c entry also has join ('separate' / 'dual' / 'chain') and,
    for 'chain', next_slab8; layers inside a dual / chained launch have no entry of their own (the next block's branch2a after a chain,
    branch1 of a dual block), conv1 is the im2col stem GEMM"""
    out = {0: run_conv(pl, bf16, 0, B, False, False, concurrent=concurrent)}
    have_2a = False
    for blk in BLOCKS:
        stg, first, last, i2a, i2b, i2c, i1 = blk
        hb = packs(pl, bf16, i2b)
        fz = use_wino_fused(pl, bf16, hb, i2b, B) or use_wino4_fused(pl, bf16, hb, i2b, B)
        if not have_2a:
            out[i2a] = run_conv(pl, bf16, i2a, B, False, False, out_slab8=fz, concurrent=concurrent)
        have_2a = False
        out[i2b] = run_conv(pl, bf16, i2b, B, False, workspace, in_slab8=fz, concurrent=concurrent)
        s2 = CONV_SPECS[i2c]
        if use_chain(pl, bf16, blk):
            nb = i2c + (3 if first else 2)
            hn = packs(pl, bf16, nb)
            out[i2c] = dict(join="chain", next_slab8=not bf16 and (use_wino_fused(pl, bf16, hn, nb, B) or use_wino4_fused(pl, bf16, hn, nb, B)))
            have_2a = True
        elif first and "w_dual" in packs(pl, bf16, i2c):
            M, N, K = B * s2.hout * s2.hout, s2.cout, s2.cin + CONV_SPECS[i1].cin
            kernel, tile = gemm_kernel(pl, bf16, DUAL, M, N, K, False, "w_dual_split" in packs(pl, bf16, i2c), concurrent)
            out[i2c] = dict(join="dual", kernel=kernel, tile=tile)
        else:
            if first:
                out[i1] = run_conv(pl, bf16, i1, B, False, False, concurrent=concurrent)
            out[i2c] = dict(run_conv(pl, bf16, i2c, B, True, False, concurrent=concurrent), join="separate")
    return out
