"""Every bf16 GEMM and conv kernel family against fp64 on the GPU, with the strict elementwise bounds of tests/kernel_check.py: each
tile code the GEMM launcher accepts with each epilogue it supports, the engine's own tile choice at every decode-step shape across
the row-count boundaries of rq_gemm_pick_tile, the implicit-GEMM conv (incl. virtual split-K) at the VAE's layer shapes, the halo
conv / conv_in / conv_out at the real high-resolution layers, and the two-phase VAE calls of a few images with RQAMD_VAE_CHUNK=1.
Outputs are views into NaN-filled guards, operands sit in NaN-poisoned buffers, and every case is launched twice (same bits)."""
import numpy as np
import pytest
import torch

import kernel_check as kc
import oracle
from oracle import configs as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CF = kc.C                              # c per kernel family (kernel_check.py); the observed values are printed at the end of each test


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    return _native


def _print_observed(prefix):
    for fam in sorted(kc.OBSERVED):
        print(f'{prefix}: {fam:10s} max err / (2^-24 n S) = {kc.OBSERVED[fam]:.4f}  (c = {CF.get(fam, 1.0)})')


def _family(bm, bn, gl):
    if (bm, bn) == (64, 32):
        return 'skinny'
    if bn == 32 or (bm, bn) == (66, 64):
        return 'stream'
    if (bm, bn) == (256, 256):
        return 'p8'
    if bm == 257:
        return 'rb'
    if bm in (132, 136, 264):
        return 'mid'
    return 'lds' if gl else 'reg'


def _tile_rows(bm):
    """rows of the tile behind a tile code (gemm.hip: 66 / 130 = the streaming kernel's 64 / 128 rows, 257 = the register-blocked 256,
    132 / 136 / 264 = the eight- / sixteen-wavefront 128 / 256)"""
    return {66: 64, 130: 128, 257: 256, 132: 128, 136: 128, 264: 256}.get(bm, bm)


def _operands(M, N, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn((M, K), device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn((N, K), device=DEV, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn((N,), device=DEV, generator=g)
    return kc.poisoned(a), kc.poisoned(w, 37), bias


class _Refs:
    """the fp64 references of one (a, w, bias) per K range, each computed once"""

    def __init__(self, a, w, bias):
        self.a, self.w, self.bias, self.cache = a, w, bias, {}

    def get(self, k0=0, k1=None, bias=True):
        key = (k0, k1, bias)
        if key not in self.cache:
            self.cache[key] = kc.gemm_ref(self.a, self.w, self.bias if bias else None, k0, k1)
        return self.cache[key]


def _launch(nat, a, w, bias, epi, bm, bn, splitk, shape, dtype, what, init=None):
    buf, out = kc.guarded(shape, dtype, DEV)
    if init is not None:
        out.copy_(init)
    nat.dbg_gemm(a, w, bias, epi=epi, bm=bm, bn=bn, splitk=splitk, out=out)
    torch.cuda.synchronize()
    kc.check_guard(buf, out.numel(), what)
    return out


def gemm_case(nat, R, kind, bm, bn, sk=1, gl=0, accum=False, extra_epi=0, family=None, x0=None):
    """one dbg_gemm case (kind 0 bf16, 1 GELU, 3 fp32, 4 slabs; accum: 4 + 2048 in place on x0), launched twice; returns the number
    of slabs written (kind 4, else 1) and the output"""
    a, w, bias = R.a, R.w, R.bias
    (M, K), N = a.shape, w.shape[0]
    family = family or _family(bm, bn, gl)
    c = CF[family]
    epi = kind + 32 * gl + (2048 if accum else 0) + extra_epi
    what = f'{family} tile {bm}x{bn} stages {gl} epi {epi} splitk {sk} M={M} N={N} K={K}'
    if kind == 4 and not accum:
        outs = [_launch(nat, a, w, None, epi, bm, bn, sk, (8, M, N), torch.float32, what) for _ in range(2)]
        written = [z for z in range(8) if not bool(torch.isnan(outs[0][z]).all())]
        ns = len(written)
        assert written == list(range(ns)) and ns >= 1, f'{what}: slabs written {written}'
        if sk > 0:
            assert ns == sk, f'{what}: {ns} slabs written'
        kc.check_nan(outs[0][ns:], what + ' (slabs past the split count)')
        bk = 32 if family == 'rb' else 64                  # K step of the kernel's loop: the unit in which it divides K over the slabs
        kt = K // bk
        per = -(-kt // ns)
        for z in range(ns):
            k0, k1 = min(z * per, kt) * bk, min((z + 1) * per, kt) * bk
            ref, S = R.get(k0, k1, bias=False)
            kc.check_f32(outs[0][z], ref, S, kc.steps(k1 - k0, ns, 0), c, what=f'{what} slab {z} (K {k0}..{k1})', family=family)
        assert torch.equal(outs[0][:ns], outs[1][:ns]), what + ': two launches differ'
        return ns, outs[0]
    ref, S = R.get()
    if accum:
        outs = [_launch(nat, a, w, bias, epi, bm, bn, sk, (M, N), torch.float32, what, init=x0) for _ in range(2)]
        kc.check_f32(outs[0], ref + x0.double(), S + x0.double().abs(), kc.steps(K, 1, 2), c, what=what, family=family)
    elif kind == 3:
        outs = [_launch(nat, a, w, bias, epi, bm, bn, sk, (M, N), torch.float32, what) for _ in range(2)]
        kc.check_f32(outs[0], ref, S, kc.steps(K, 1, 1), c, what=what, family=family)
    else:
        outs = [_launch(nat, a, w, bias, epi, bm, bn, sk, (M, N), torch.bfloat16, what) for _ in range(2)]
        kc.check_bf16(outs[0], ref, S, kc.steps(K, 1, 1), c, gelu=kind == 1, what=what, family=family)
    assert torch.equal(outs[0], outs[1]), what + ': two launches differ'
    return 1, outs[0]


# ------------------------------------------------------------------------------------------------ B.1: every tile code
# (tile code, LDS-DMA stages): every combination rq_gemm_launch accepts (gemm.hip)
TILES = [((64, 32), 0),                                                    # skinny (M <= 64, in-workgroup split-K)
         ((66, 32), 0), ((130, 32), 0), ((66, 64), 0),                     # weight-streaming kernel, 64 / 128 rows x 32 / 64 weight rows
         ((64, 64), 0), ((64, 128), 0), ((128, 64), 0), ((128, 128), 0), ((256, 128), 0),      # register-staged
         ((128, 64), 2), ((128, 64), 3), ((128, 128), 2), ((128, 128), 3), ((256, 128), 2), ((256, 128), 3),   # LDS-DMA
         ((257, 128), 2), ((257, 128), 3),                                 # register-blocked 256 x 128 (BK 32)
         ((132, 64), 3), ((136, 128), 3), ((132, 192), 3), ((264, 128), 3), ((136, 256), 3),   # mid-batch eight / sixteen wavefronts
         ((256, 256), 0)]                                                  # eight-phase 256 x 256


def _tile_shapes(code):
    """(M, N, K, K splits) per tile: M and N one above / one below a tile multiple, odd N (scalar epilogue stores) and N % 8 == 4
    (4-wide, not 8-wide stores), an even (24) and an odd (15) K-tile count, and >= 8 n-tiles over 6 m-tiles (n-ranges per XCD; the
    K-slice schedule 4 of the LDS-DMA slab GEMMs)"""
    bm, bn = code
    if code == (64, 32):                                                    # (K / splitk) % 512 == 0
        return [(63, 3 * 32 - 1, 1536, (1, 3)), (33, 36, 2048, (1, 2, 4))]
    BM, BN = _tile_rows(bm), bn
    # (15 K-tiles in 6 splits would leave the last slab empty -- no picker asks for that)
    shapes = [(2 * BM + 1, 3 * BN - 1, 1536, (1, 2, 3, 4, 6, 8)), (BM - 1, BN + 4, 960, (1, 2, 3, 4, 8)),
              (5 * BM + 1, 8 * BN + 4, 1536, (1, 2, 4, 8))]
    if code == (256, 256):                                                  # >= 2 K-tiles per split, K-tiles % splits == 0
        shapes[1] = (BM - 1, BN + 4, 960, (1, 3))
    return shapes


@pytest.mark.parametrize('code,gl', TILES, ids=[f'{c[0]}x{c[1]}_gl{g}' for c, g in TILES])
def test_gemm_tile_matrix(nat, code, gl):
    """dbg_gemm with an explicit tile: bf16, GELU, fp32, split-K slabs (every accepted split count, each slab against its own K range)
    and the in-place residual epilogue (N % 4 == 0 only; refused otherwise) -- vs fp64."""
    bm, bn = code
    kc.OBSERVED.clear()
    phases = (512, 1024) if code == (256, 256) else (0,)                   # the eight-phase kernel: 2 and 4 phases per K-tile
    for si, (M, N, K, splits) in enumerate(_tile_shapes(code)):
        a, w, bias = _operands(M, N, K, 100 + si)
        R = _Refs(a, w, bias)
        x0 = torch.randn((M, N), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
        for ph in phases:
            for kind in (0, 1, 3):
                gemm_case(nat, R, kind, bm, bn, 1, gl, extra_epi=ph)
            for sk in splits:
                gemm_case(nat, R, 4, bm, bn, sk, gl, extra_epi=ph)
            if N % 4 == 0 and code != (64, 32):
                gemm_case(nat, R, 4, bm, bn, 1, gl, accum=True, extra_epi=ph, x0=x0)
            else:
                buf, out = kc.guarded((M, N), torch.float32, DEV)
                with pytest.raises(ValueError):
                    nat.dbg_gemm(a, w, bias, epi=4 + 2048 + 32 * gl + ph, bm=bm, bn=bn, splitk=1, out=out)
                kc.check_nan(buf, 'refused launch')
        del R
    if code in ((128, 64), (257, 128)) and gl in (0, 2):
        # the m-band schedule (gemm.hip launch_c / launch_rb: >= 8 m- and n-tiles, activations much larger than the weights)
        M, N, K = (5121, 508, 2048) if bm == 128 else (4097, 1020, 3072)
        a, w, bias = _operands(M, N, K, 120)
        R = _Refs(a, w, bias)
        for kind in (0, 3):
            gemm_case(nat, R, kind, bm, bn, 1, gl)
        del R
    _print_observed(f'tile {bm}x{bn} stages {gl}')


def test_gemm_refusals(nat):
    """The documented refusals raise (and store nothing) instead of launching: afterwards the library still computes correctly."""
    def refused(exc, a, w, bias, epi, bm, bn, sk, shape, dtype=torch.float32):
        buf, out = kc.guarded(shape, dtype, DEV)
        with pytest.raises(exc):
            nat.dbg_gemm(a, w, bias, epi=epi, bm=bm, bn=bn, splitk=sk, out=out)
        torch.cuda.synchronize()
        kc.check_nan(buf, f'refused epi {epi} tile {bm}x{bn} splitk {sk}')
    a, w, bias = _operands(256, 256, 64, 1)
    refused(NotImplementedError, a, w, bias, 3, 256, 256, 1, (256, 256))                # 256 x 256 with one K-tile
    a, w, bias = _operands(256, 256, 192, 2)
    refused(NotImplementedError, a, w, None, 4, 256, 256, 2, (8, 256, 256))             # 256 x 256: 3 K-tiles in 2 splits
    a, w, bias = _operands(65, 128, 1024, 3)
    refused(NotImplementedError, a, w, bias, 3, 64, 32, 1, (65, 128))                   # skinny: M > 64
    a, w, bias = _operands(64, 128, 1024, 4)
    refused(NotImplementedError, a, w, None, 4, 64, 32, 4, (8, 64, 128))                # skinny: 256 K per split
    refused(ValueError, a, w, bias, 4 + 2048, 64, 32, 1, (64, 128))                     # skinny: no in-place epilogue
    refused(ValueError, a, w, bias, 4 + 2048, 128, 64, 2, (64, 128))                    # in place with a K split
    refused(ValueError, a, w, bias, 3, 128, 64, 2, (64, 128))                           # K split without slabs
    refused(ValueError, a, w, bias, 3, 96, 96, 1, (64, 128))                            # no such tile
    a, w, bias = _operands(64, 130, 1024, 5)
    refused(ValueError, a, w, bias, 4 + 2048, 128, 64, 1, (64, 130))                    # in place with N % 4 != 0
    # the conv form: no streaming tile, virtual split-K only with an even number of K-tiles per chunk and the 256-row tile as 256 x 128
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn((1, 8, 8, 128), device=DEV, generator=g).to(torch.bfloat16)
    wc = (0.05 * torch.randn((128, 3, 3, 128), device=DEV, generator=g)).to(torch.bfloat16)
    for exc, bm, bn, flags in ((NotImplementedError, 66, 32, 0), (ValueError, 128, 128, 2 << 8), (ValueError, 128, 128, 4 << 8)):
        buf, out = kc.guarded((1, 8, 8, 128), torch.bfloat16, DEV)
        with pytest.raises(exc):
            nat.dbg_conv(x, wc, None, bm=bm, bn=bn, flags=flags, out=out)       # 18 K-tiles: 2 x 9 (odd), 4 x 4.5
        torch.cuda.synchronize()
        kc.check_nan(buf, f'refused conv {bm}x{bn} flags {flags}')
    # after the refusals: a valid launch
    a, w, bias = _operands(200, 192, 320, 8)
    kc.OBSERVED.clear()
    gemm_case(nat, _Refs(a, w, bias), 3, 128, 64)


# ------------------------------------------------------------------------------------------------ B.2: the engine's own choice
def pick_tile(M, N, K, slab):
    """rq_gemm_pick_tile (gemm.hip) with the LDS-DMA kernels allowed and no A/B switches: (tile code bm, bn, K splits, LDS stages)"""
    def cdiv(a, b):
        return -(-a // b)
    kt = K // 64
    if M <= 128 and (N < 16384 or (M <= 64 and N == 16384)) and N >= 64:
        bm, bn, sk = (66 if M <= 64 else 130), 32, 1
        if slab:
            nt = cdiv(N, 32)
            while sk < 8 and nt * sk * 2 <= 256 and kt % (sk * 2) == 0 and kt // (sk * 2) >= 4:
                sk *= 2
        if M <= 64:
            nt32, nt64 = cdiv(N, 32), cdiv(N, 64)
            if nt32 > 256:
                bn = 64
            elif slab and kt >= 32 and nt32 * 4 > 256 and nt64 * 4 <= 256 and kt % 4 == 0:
                bn, sk = 64, 4
        return bm, bn, sk, 0
    if 128 < M < 2048 and N >= 64:
        wide = not slab and N >= 8192
        if wide and M > 256:
            if M < 1024:
                return 136, 256, 1, 3
        else:
            best = None
            for code, BM, BN in ((132, 128, 64), (136, 128, 128), (132, 128, 192), (264, 256, 128), (136, 128, 256)):
                MT, NT = cdiv(M, BM), cdiv(N, BN)
                for sk in ((1, 2, 3, 4, 6, 8) if slab else (1,)):
                    if kt % sk != 0 or (sk > 1 and kt // sk < 4):
                        continue
                    Wg = float(MT * NT * sk)
                    bw = float(BM + BN) * 128.0 * (kt // sk)
                    wx = (cdiv(NT, 8) * MT * sk) if NT >= 8 else (cdiv(MT, 8) * NT * sk)
                    rounds = (wx + 31) // 32
                    ts = max(rounds * bw / 110e3, Wg * bw / 17e6)
                    tm = rounds * 2.0 * BM * BN * float(K) / sk / 5e6
                    t = 2.0 + max(ts, tm) + 0.4 * min(ts, tm) + 2.5 + float(BM) * BN * (4 if (slab or wide) else 2) / 32e3
                    if slab and sk > 1:
                        t += sk * float(M) * N * 4.0 / 4.5e6
                    if best is None or t < best[0]:
                        best = (t, code, BN, sk)
            if best is not None:
                return best[1], best[2], best[3], 3
    if M >= 2048 and kt >= 2:
        MT, NT = cdiv(M, 256), cdiv(N, 256)
        tiles = MT * NT
        t_epi = 8.0 if slab else 6.0
        best, bsk, sk = 1e30, 1, 1
        while sk <= (4 if slab else 1):
            if not (sk > 1 and (kt % sk != 0 or kt // sk < 12)):
                wgs = tiles * sk
                full, rem = wgs // 256, wgs % 256
                nkp = kt // sk
                t = 4.0 + full * (nkp * 1.5 + t_epi)
                if rem:
                    t += nkp * (1.05 + 0.45 * rem / 256.0) + t_epi
                if sk > 1:
                    t += 6.0 * (sk - 1)
                if t < best:
                    best, bsk = t, sk
            sk *= 2
        if best < 2.0 * M * float(N) * K / 1e6 / (650.0 if slab else 750.0):
            return 256, 256, bsk, 2
    if M >= 512:
        if N >= 16384:
            if M >= 4096:
                return 257, 128, 1, 2
            return 256, 128, 1, 3 if M < 2048 else 2
        if M >= 8192:
            return (257, 128, 1, 2) if N >= 6144 else (128, 128, 1, 2)
        if M >= 4096 and N >= 4096:
            return 128, 128, 1, 2
        if M >= 2048 and slab and K >= 4096 and N <= 2048:
            return 256, 128, 1 if M >= 4096 else 2, 3
        maxsplit = min(max(kt // 8, 1), 8) if slab else 1
        return 128, 64, min(max(cdiv(768, cdiv(M, 128) * cdiv(N, 64)), 1), maxsplit), 2
    maxsplit = min(max(kt // 8, 1), 8) if slab else 1
    if M >= 2048 and cdiv(N, 128) % 8 == 0 and cdiv(M, 256) * cdiv(N, 128) >= 192:
        return 256, 128, 1, 0
    cand = ((128, 128), (128, 64), (64, 128), (64, 64))
    pick = 3
    for ci, (cm, cn) in enumerate(cand):
        if M <= 64 and cm > 64:
            continue
        nt = cdiv(N, cn)
        if nt >= 8 and (nt & 7) != 0 and cdiv(N, 64) % 8 == 0:
            continue
        if cdiv(M, cm) * nt * maxsplit >= 512:
            pick = ci
            break
    bm, bn = cand[pick]
    return bm, bn, min(max(cdiv(768, cdiv(M, bm) * cdiv(N, bn)), 1), maxsplit), 0


# E and the classifier's vocabulary of the released stage-2 models (oracle/configs.py): FFHQ 355M, CC3M 654M (its text classifier has
# the same 16384 x 1280 shape), ImageNet 480M .. 1.4B, ImageNet 3.8B / the 3.9B text model
MODELS = [(1024, 2048), (1280, 16384), (1536, 16384), (2560, 16384)]
# decode-step row counts, with the picker branch each boundary crosses (gemm.hip rq_gemm_pick_tile)
ROWS = [1, 2, 31, 33,      # weight-streaming kernel, 64-row form; the K split count for the slab GEMMs; 64-row weight tiles at E = 2560
        63, 64, 65,        # 64 | 65: 128-row streaming form; the classifier (N = 16384) leaves it for the register-staged 64 x 64 tiles
        127, 128, 129,     # 128 | 129: the mid-batch cost model over the eight- / sixteen-wavefront LDS-DMA tiles and their K splits
        255, 257,          # 256 | 257: the classifier's wide fp32 rows take the 136 x 256 tile
        500, 511, 512,     # (500: the reference's metric batch)
        1023, 1024,        # 1023 | 1024: the classifier goes to the 256 x 128 LDS-DMA tile
        2047, 2048, 2049,  # 2047 | 2048: the mid-batch model ends; the 256 x 256 cost model against the LDS-DMA rules (fc2: 256 x 128 / 2 splits)
        4095, 4096,        # 4095 | 4096: the classifier's register-blocked 257 tile, qkv / fc1 128 x 128, fc2 one split
        8191, 8192,        # 8191 | 8192: register-blocked tile for N >= 6144, 128 x 128 otherwise (where the 256 x 256 model declines)
        10752]             # bench.py's decode rows


def _step_gemms(E, V):
    """(name, N, K, kind) of every GEMM step_gemm issues (engine_rqt.hip): qkv, proj (slabs), fc1 (GELU), fc2 (slabs), the input
    embedding (fp32, K = input_embed_dim 256) and the classifier (fp32)"""
    return [('qkv', 3 * E, E, 0), ('proj', E, E, 4), ('fc1', 4 * E, E, 1), ('fc2', E, 4 * E, 4), ('embed', E, 256, 3), ('cls', V, E, 3)]


def _same_as_modelled(nat, a, w, bias, kind, pick, auto, what):
    """the explicit launch of the tile, split count and stages pick_tile models gives the bits of the engine's own choice (auto): the
    family each case is judged as, and the families the coverage assertion counts, are the library's, not only the model's"""
    bm, bn, sk, gl = pick
    what = f'{what}: modelled pick {bm}x{bn} splitk {sk} stages {gl}'
    explicit = _launch(nat, a, w, None if kind == 4 else bias, kind + 32 * gl, bm, bn, sk, tuple(auto.shape), auto.dtype, what)
    if kind == 4:
        kc.check_nan(explicit[sk:], what)
        explicit, auto = explicit[:sk], auto[:sk]
    assert torch.equal(explicit, auto), what + ": not the bits of the engine's own choice"


@pytest.mark.parametrize('E,V', MODELS, ids=[f'E{e}' for e, _ in MODELS])
def test_gemm_engine_choice(nat, E, V):
    """dbg_gemm with bm = bn = 0, splitk = 0: the engine's tile / split choice at every step_gemm shape and row count, vs fp64; the slab
    count written (found from the NaN prefill) is the one pick_tile models, each slab holds its own K range, the launch of the modelled
    tile gives the same bits, and where the pick is one slab the fused residual path (4 + 2048, splitk 1: engine_rqt.hip step_gemm) as
    well."""
    kc.OBSERVED.clear()
    seen = set()
    for M in ROWS:
        for (name, N, K, kind) in _step_gemms(E, V):
            bm, bn, sk, gl = pick_tile(M, N, K, kind == 4)
            fam = _family(bm, bn, gl)
            seen.add(fam)
            a, w, bias = _operands(M, N, K, M * 7 + N)
            R = _Refs(a, w, bias)
            ns, auto = gemm_case(nat, R, kind, 0, 0, 0, family=fam)
            if kind == 4:
                assert ns == sk, f'{name} M={M}: {ns} slabs written, the picker model says {sk} ({bm}x{bn})'
            _same_as_modelled(nat, a, w, bias, kind, (bm, bn, sk, gl), auto, f'{name} M={M}')
            del auto
            if kind == 4 and ns == 1:
                x0 = torch.randn((M, N), device=DEV, generator=torch.Generator(device=DEV).manual_seed(M))
                gemm_case(nat, R, 4, 0, 0, 1, accum=True, family=fam, x0=x0)
            del R, a, w
    # the register-blocked 257 x 128 tile: what the picker returns for wide fp32 rows from 4096 rows on where the 256 x 256 model declines --
    # at none of the shapes above (its cost model wins there), so a short-K classifier shape
    assert pick_tile(4096, 16384, 128, False) == (257, 128, 1, 2)
    a, w, bias = _operands(4096, 16384, 128, E)
    _, auto = gemm_case(nat, _Refs(a, w, bias), 3, 0, 0, 0, family='rb')
    _same_as_modelled(nat, a, w, bias, 3, (257, 128, 1, 2), auto, 'rb probe')
    seen.add('rb')
    del a, w
    _print_observed(f'engine choice E={E}')
    # (the register-staged tiles: the 16384-word classifier at 65 .. 128 rows)
    assert seen == {'stream', 'mid', 'p8', 'lds', 'rb'} | ({'reg'} if V >= 16384 else set()), seen


# ------------------------------------------------------------------------------------------------ C.1 / C.2: implicit-GEMM conv
# (label, H, Cin, Cout, stride, ups) of every 3x3 conv engine_vae.hip runs as an implicit GEMM for VAE_IMAGENET / VAE_FFHQ (the same conv
# shapes; H = the conv's input size, after the folded upsample)
CONV_LAYERS = [('encoder.down.0.downsample', 256, 128, 128, 2, 0), ('encoder.down.1.downsample', 128, 128, 128, 2, 0),
               ('encoder.down.2.downsample', 64, 256, 256, 2, 0), ('encoder.down.3.downsample', 32, 256, 256, 2, 0),
               ('encoder.down.4.downsample', 16, 512, 512, 2, 0),
               ('encoder.down.4.block.0.conv1', 16, 256, 512, 1, 0), ('16^2 512 -> 512', 16, 512, 512, 1, 0),
               ('8^2 512 -> 512', 8, 512, 512, 1, 0), ('decoder.conv_in', 8, 256, 512, 1, 0), ('encoder.conv_out', 8, 512, 256, 1, 0),
               ('decoder.up.5.upsample', 16, 512, 512, 1, 1),
               # the 32^2 layers that RQAMD_HALO_LOWRES=0 routes here
               ('32^2 256 -> 256', 32, 256, 256, 1, 0), ('decoder.up.3.block.0.conv1', 32, 512, 256, 1, 0),
               ('decoder.up.4.upsample', 32, 512, 512, 1, 1)]
CONV_TILES = [(64, 64), (64, 128), (128, 64), (128, 128), (256, 128)]


def engine_conv_tile(M, Cout):
    """engine_vae.hip VaeRun::conv: 128 rows from 128 output pixels, 128 columns where Cout allows, the 8-wave 256-row tile for the big layers"""
    bm, bn = (128 if M >= 128 else 64), (128 if Cout % 128 == 0 else 64)
    if bn == 128 and (M // 256) * (Cout // 128) >= 512:
        bm = 256
    return bm, bn


def k_split(kt):
    """engine_vae.hip VaeRun::k_split"""
    for sk in range(16, 1, -1):
        if kt % (2 * sk) == 0 and kt // sk >= 4:
            return sk
    return 1


def _conv_case(nat, x, w, bias, resid, stride, ups, bm, bn, vs, ref, S, what):
    B, Cout = x.shape[0], w.shape[0]
    H, W = x.shape[1] << ups, x.shape[2] << ups
    Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
    outs = []
    for _ in range(2):
        buf, out = kc.guarded((B, Ho, Wo, Cout), torch.bfloat16, DEV)
        nat.dbg_conv(x, w, bias, resid, ksize=3, stride=stride, ups=ups, bm=bm, bn=bn, flags=vs << 8, out=out)
        torch.cuda.synchronize()
        kc.check_guard(buf, out.numel(), what)
        outs.append(out)
    K = 9 * w.shape[3]
    kc.check_bf16(outs[0].reshape(-1, Cout), ref, S, kc.steps(K, vs, 2 if resid is not None else 1), CF['conv'], what=what, family='conv')
    assert torch.equal(outs[0], outs[1]), what + ': two launches differ'


@pytest.mark.parametrize('layer', CONV_LAYERS, ids=[c[0] for c in CONV_LAYERS])
def test_conv_implicit_gemm_layers(nat, layer):
    """dbg_conv at the VAE's implicit-GEMM layers, B = 1 / 3 / 9, with and without residual, the engine's tile and every other conv tile;
    on the <= 32^2 layers also with the engine's virtual split-K count (flags bits 8..12) -- vs an fp64 im2col reference."""
    label, H, Cin, Cout, stride, ups = layer
    kc.OBSERVED.clear()
    Ho = H // 2 if stride == 2 else H
    kt = 9 * Cin // 64
    vsplit = k_split(kt) if Ho * Ho <= 1024 and kt >= 16 else 1
    for B in (1, 3, 9):
        g = torch.Generator(device=DEV).manual_seed(B * 1000 + H + Cin)
        x = kc.poisoned(torch.randn((B, H >> ups, H >> ups, Cin), device=DEV, generator=g).to(torch.bfloat16), 1)
        w = kc.poisoned((torch.randn((Cout, 3, 3, Cin), device=DEV, generator=g) / (9 * Cin) ** 0.5).to(torch.bfloat16), 5)
        bias = torch.randn((Cout,), device=DEV, generator=g)
        resid = kc.poisoned(torch.randn((B, Ho, Ho, Cout), device=DEV, generator=g).to(torch.bfloat16), 1)
        ref, S, _ = kc.conv_ref(x, w, bias, stride=stride, ups=ups)
        M = B * Ho * Ho
        etile = engine_conv_tile(M, Cout)
        for r in (None, resid):
            rr, rS = (ref, S) if r is None else (ref + r.double().reshape(-1, Cout), S + r.double().abs().reshape(-1, Cout))
            for (bm, bn) in [etile] + [t for t in CONV_TILES if t != etile]:
                for vs in ((1, vsplit) if vsplit > 1 else (1,)):
                    what = f'{label} B={B} tile {bm}x{bn} vsplit {vs} resid {r is not None}'
                    _conv_case(nat, x, w, bias, r, stride, ups, bm, bn, vs, rr, rS, what)
            del rr, rS
        del ref, S
    _print_observed(label)


# the 1x1 convs: dense GEMMs in the engine (conv = 0), its explicit tile, no LDS-DMA stages; (label, H, Cin, Cout, kind)
DENSE_1X1 = [('post_quant_conv', 8, 256, 256, 0), ('quant_conv', 8, 256, 256, 3), ('encoder.down.4.block.0.nin_shortcut', 16, 256, 512, 0),
             ('decoder.up.3.block.0.nin_shortcut', 32, 512, 256, 0), ('encoder.down.2.block.0.nin_shortcut', 64, 128, 256, 0),
             ('decoder.up.1.block.0.nin_shortcut', 128, 256, 128, 0)]


def test_conv_1x1_dense(nat):
    kc.OBSERVED.clear()
    for (label, H, Cin, Cout, kind) in DENSE_1X1:
        for B in (1, 3, 9):
            M = B * H * H
            a, w, bias = _operands(M, Cout, Cin, M + Cout)
            bm, bn = engine_conv_tile(M, Cout)
            gemm_case(nat, _Refs(a, w, bias), kind, bm, bn, 1, 0)
    _print_observed('1x1 convs')


# ------------------------------------------------------------------------------------------------ C.3: halo conv, conv_in, conv_out
# (H, Cin, Cout) of the 3x3 / stride-1 layers the halo kernel runs at 256^2 .. 32^2 (decoder and encoder)
HALO_LAYERS = [(256, 128, 128), (128, 128, 128), (128, 256, 128), (64, 128, 256), (64, 256, 256), (32, 256, 256), (32, 512, 256)]
# the upsample convs into 256^2 .. 32^2: (H out, C)
HALO_UPS = [(256, 128), (128, 256), (64, 256), (32, 512)]


def _halo_case(nat, x, w, bias, ref, S, extra, what, taps=9, **kw):
    B, Cout = x.shape[0], w.shape[0]
    H, W = (x.shape[1] * 2, x.shape[2] * 2) if kw.get('ups') else (x.shape[1], x.shape[2])
    outs = []
    for _ in range(2):
        buf, out = kc.guarded((B, H, W, Cout), torch.bfloat16, DEV)
        nat.dbg_conv_halo(x, w, bias, out=out, **kw)
        torch.cuda.synchronize()
        kc.check_guard(buf, out.numel(), what)
        outs.append(out)
    n = kc.steps(taps * w.shape[3], 1, 2 if kw.get('resid') is not None else 1)
    kc.check_bf16(outs[0].reshape(-1, Cout), ref, S, n, CF['halo'], extra=extra, what=what, family='halo')
    assert torch.equal(outs[0], outs[1]), what + ': two launches differ'
    return outs[0]


def _check_partials(stats, s1, sa, s2, terms, what):
    """GroupNorm partials (B, P, 32, 2) against fp64 sums of their `terms` bf16 outputs each (s1 = sum, sa = sum |.|, s2 = sum of squares,
    (B, P, 32)).  Not the measured-c rule of the rest of this file: a fixed worst-case bound for sequential fp32 summation, c = 1 with n =
    the number of terms (+ 1 for the squares' own rounding).  The observed ratio is printed ('stats') so that it can be tightened."""
    kc.check_f32(stats[..., 0], s1, sa, terms + 1, 1.0, what=what + ' stats sum', family='stats')
    kc.check_f32(stats[..., 1], s2, s2, terms + 2, 1.0, what=what + ' stats sum of squares', family='stats')


def _check_stats(stats, out, what):
    """per (8 x 32 output tile, group) sum and sum of squares of the bf16 output (the per-tile form), see _check_partials"""
    B, H, W, Cout = out.shape
    t = out.double().reshape(B, H // 8, 8, W // 32, 32, 32, Cout // 32)
    s1, sa, s2 = t.sum((2, 4, 6)), t.abs().sum((2, 4, 6)), (t * t).sum((2, 4, 6))
    _check_partials(stats, s1.reshape(B, -1, 32), sa.reshape(B, -1, 32), s2.reshape(B, -1, 32), 8 * 32 * (Cout // 32), what)


def test_halo_conv_real_layers(nat):
    """The halo-reuse conv at the decoder / encoder layers (B = 2): plain, fused GroupNorm + SiLU with residual and epilogue statistics,
    and the upsample convs in the per-tile and the sub-pixel form (the latter against the fp64 2 x 2 convs with the library's own
    pre-summed bf16 taps, its statistics per output lattice) -- vs fp64.  With the fused GroupNorm the reference rounds
    silu(x gamma + beta) to bf16 as the kernel does, and |W| * ulp(xn) is added to the bound (kernel and torch may round one input
    differently)."""
    kc.OBSERVED.clear()
    B = 2
    for (H, Cin, Cout) in HALO_LAYERS:
        g = torch.Generator(device=DEV).manual_seed(H + Cin + Cout)
        x = kc.poisoned(torch.randn((B, H, H, Cin), device=DEV, generator=g).to(torch.bfloat16), 1)
        w = kc.poisoned((torch.randn((Cout, 3, 3, Cin), device=DEV, generator=g) / (9 * Cin) ** 0.5).to(torch.bfloat16), 5)
        bias = torch.randn((Cout,), device=DEV, generator=g)
        resid = kc.poisoned(torch.randn((B, H, H, Cout), device=DEV, generator=g).to(torch.bfloat16), 1)
        gn = torch.stack([1.0 + 0.2 * torch.randn((B, Cin), device=DEV, generator=g), 0.3 * torch.randn((B, Cin), device=DEV, generator=g)], -1).contiguous()
        what = f'halo {H}^2 {Cin}->{Cout}'
        ref, S, _ = kc.conv_ref(x, w, bias)
        _halo_case(nat, x, w, bias, ref, S, None, what + ' plain')
        del ref, S
        xn = torch.nn.functional.silu(x.float() * gn[:, None, None, :, 0] + gn[:, None, None, :, 1]).to(torch.bfloat16)
        ref, S, extra = kc.conv_ref(xn, w, bias, resid=resid, xulp=kc.bf16_ulp(xn.double()))
        stats = torch.full((B, (H // 8) * (H // 32), 32, 2), float('nan'), device=DEV)
        out = _halo_case(nat, x, w, bias, ref, S, extra, what + ' gn+silu+resid', gn=gn, resid=resid, stats=stats)
        _check_stats(stats, out, what)
        del ref, S, extra, xn
    for (H, Cc) in HALO_UPS:
        g = torch.Generator(device=DEV).manual_seed(H * 3 + Cc)
        xs = kc.poisoned(torch.randn((B, H // 2, H // 2, Cc), device=DEV, generator=g).to(torch.bfloat16), 1)
        w = kc.poisoned((torch.randn((Cc, 3, 3, Cc), device=DEV, generator=g) / (9 * Cc) ** 0.5).to(torch.bfloat16), 5)
        bias = torch.randn((Cc,), device=DEV, generator=g)
        ref, S, _ = kc.conv_ref(xs, w, bias, ups=1)
        what = f'halo upsample into {H}^2 {Cc}'
        _halo_case(nat, xs, w, bias, ref, S, None, what + ' per-tile', ups=True)
        del ref, S
        if (H // 2) % 8 == 0 and (H // 2) % 32 == 0:
            # sub-pixel form: four 2 x 2 convs over the source image with pre-summed bf16 taps.  The taps are the library's own
            # (dbg_ups_subpixel_weights: each the RNE bf16 of its fp32 tap sum, checked here against the fp64 sum), the reference is
            # the fp64 2 x 2 conv with exactly those taps -- the same strict bound as every other case
            wsub = nat.dbg_ups_subpixel_weights(w)
            taps = kc.subpixel_taps64(w)
            terr = (wsub.double() - taps).abs()
            assert bool((terr <= 0.5 * kc.bf16_ulp(taps) + kc.U * taps.abs()).all()), what + ': pre-summed taps are not the rounded sums'
            ref, S = kc.subpixel_conv_ref(xs, wsub, bias)
            stats = torch.full((B, (H // 8) * (H // 32), 32, 2), float('nan'), device=DEV)
            out = _halo_case(nat, xs, w, bias, ref, S, None, what + ' sub-pixel', taps=4, ups=True, subpixel=True,
                             stats=stats)
            del ref, S, wsub, taps, terr
            # one partial per (8 x 32 source tile, output parity class (py, px)) = the sums over that 8 x 32 lattice of output pixels:
            # partial 4 tile + 2 py + px of the image (conv_halo.hip HaloTile::trem), each against its own lattice
            lat = out.double().reshape(B, H // 16, 8, 2, H // 64, 32, 2, 32, Cc // 32).permute(0, 1, 4, 3, 6, 2, 5, 7, 8)
            lat = lat.reshape(B, -1, 8 * 32, 32, Cc // 32)
            _check_partials(stats, lat.sum((2, 4)), lat.abs().sum((2, 4)), (lat * lat).sum((2, 4)), 8 * 32 * (Cc // 32), what + ' sub-pixel')
            del lat
    _print_observed('halo')


def _conv_in_guarded(nat, x, w, bias):
    """rqamd_dbg_conv_in_bf16 into a NaN-guarded output (the wrapper allocates its own)"""
    B, _, H, W = x.shape
    buf, y = kc.guarded((B, H, W, 128), torch.bfloat16, DEV)
    nat.check(nat.lib().rqamd_dbg_conv_in_bf16(nat.ptr(x, torch.float32), nat.ptr(w, torch.float32), nat.ptr(bias, torch.float32),
                                               B, H, W, nat.ptr(y), nat.stream_of(x)))
    torch.cuda.synchronize()
    kc.check_guard(buf, y.numel(), 'conv_in')
    return y


def _conv_out_guarded(nat, x, w, bias, gn):
    """rqamd_dbg_conv_out_bf16 into a NaN-guarded output (the wrapper allocates its own)"""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    buf, y = kc.guarded((B, Cout, H, W), torch.float32, DEV)
    nat.check(nat.lib().rqamd_dbg_conv_out_bf16(nat.ptr(x, torch.bfloat16), nat.ptr(w, torch.float32), nat.ptr(bias, torch.float32),
                                                nat.ptr(gn), B, H, W, Cin, Cout, nat.ptr(y), nat.stream_of(x)))
    torch.cuda.synchronize()
    kc.check_guard(buf, y.numel(), 'conv_out')
    return y


def test_conv_in_out_real_layers(nat):
    """The MFMA Encoder.conv_in (3 -> 128, NCHW fp32 in) and Decoder.conv_out (128 -> 3, NCHW fp32 out, with / without the fused
    norm_out + swish) at 256^2, B = 3 -- vs fp64; outputs inside NaN guards, image / weights / bias / GroupNorm parameters with NaN
    behind their ends."""
    kc.OBSERVED.clear()
    g = torch.Generator(device=DEV).manual_seed(31)
    B, H = 3, 256
    x = kc.poisoned(torch.randn((B, 3, H, H), device=DEV, generator=g).clamp(-1, 1), 1)
    w = 0.2 * torch.randn((128, 3, 3, 3), device=DEV, generator=g)
    bias = kc.poisoned(torch.randn((128,), device=DEV, generator=g), 32)
    wk = kc.poisoned(w.permute(2, 3, 1, 0).contiguous(), 1)                          # (ky, kx, ci, cout)
    xb, wb = x.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous(), w.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
    ref, S, _ = kc.conv_ref(xb, wb, bias)
    outs = [_conv_in_guarded(nat, x, wk, bias) for _ in range(2)]
    kc.check_bf16(outs[0].reshape(-1, 128), ref, S, kc.steps(27, 1, 1), CF['conv_in'], what='conv_in 256^2', family='conv_in')
    assert torch.equal(outs[0], outs[1])
    del ref, S
    Cin = 128
    x = kc.poisoned(torch.randn((B, H, H, Cin), device=DEV, generator=g).to(torch.bfloat16), 1)
    w = kc.poisoned(0.05 * torch.randn((3, 3, 3, Cin), device=DEV, generator=g), 1)
    bias = kc.poisoned(torch.randn((3,), device=DEV, generator=g), 13)
    gn = kc.poisoned(torch.stack([1.0 + 0.2 * torch.randn((B, Cin), device=DEV, generator=g),
                                  0.3 * torch.randn((B, Cin), device=DEV, generator=g)], -1).contiguous(), 1)
    wb = w.to(torch.bfloat16)
    for use_gn in (False, True):
        xin, xulp = x, None
        if use_gn:
            xin = torch.nn.functional.silu(x.float() * gn[:, None, None, :, 0] + gn[:, None, None, :, 1]).to(torch.bfloat16)
            xulp = kc.bf16_ulp(xin.double())
        ref, S, extra = kc.conv_ref(xin, wb, bias, xulp=xulp)
        outs = [_conv_out_guarded(nat, x, w, bias, gn if use_gn else None) for _ in range(2)]
        got = outs[0].permute(0, 2, 3, 1).reshape(-1, 3)
        kc.check_f32(got, ref, S, kc.steps(9 * Cin, 1, 1), CF['conv_out'], extra=extra, what=f'conv_out 256^2 gn={use_gn}', family='conv_out')
        assert torch.equal(outs[0], outs[1])
        del ref, S, extra
    _print_observed('conv_in / conv_out')


# ------------------------------------------------------------------------------------------------ D: two-phase calls of few images
def test_vae_two_phase_chunk1_reserves_its_split_k_slab(nat, monkeypatch):
    """With RQAMD_VAE_CHUNK=1 a call of 6 .. 9 images runs its <= 16^2 layers over a super-chunk of up to 8 images, which takes the
    split-K slab path (<= SPLIT_MAX_B images) and needs the slab sized for the super-chunk, not for the 1-image chunk (used to fail with
    'split-K slab ... was not reserved').  Same bits as the default chunking."""
    from rqvae.models.rqvae import RQVAE
    hps, dd = C.VAE_IMAGENET
    params = {k: torch.from_numpy(v) for k, v in oracle.make_params(oracle.rqvae_param_shapes(hps, dd), 5).items()}

    def model():
        m = RQVAE(**hps, ddconfig=dd, checkpointing=False)
        m.load_state_dict(params, strict=True)
        return m.to(DEV).eval()
    rng = np.random.default_rng(9)
    codes = torch.from_numpy(rng.integers(0, 16384, (9, 8, 8, 4))).to(DEV)
    x = torch.from_numpy(np.clip(rng.standard_normal((9, 3, 256, 256), dtype=np.float32), -1, 1)).to(DEV)
    vae0 = model()
    d0, z0 = vae0.decode_code(codes), vae0.encode(x)
    monkeypatch.setenv('RQAMD_VAE_CHUNK', '1')             # read when the engine is created
    vae1 = model()
    for n in (6, 7, 8, 9):
        assert torch.equal(vae1.decode_code(codes[:n].clone()), d0[:n]), n
        assert torch.equal(vae1.encode(x[:n].clone()), z0[:n]), n
