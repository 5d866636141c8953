"""AttnBlock's attention beyond 64 tokens on a real MI355X (`-m gpu`): vae_attn_tiled_kernel alone through rqamd_dbg_vae_attn against fp64,
and RQ-VAEs with 16 x 16, 32 x 32 and 64 x 64 latents end to end against fixtures made by the reference (tests/golden/vae_map*.npz,
tests/golden/make_golden_vae_maps.py).

Stand-alone bound (tests/vae_attn_cases.py): |out - ref| <= 1/2 ulp_bf16(ref) + c 2^-17 A elementwise, c = C_BOUND = 0.4 = 3 x the largest
(err - 1/2 ulp) / (2^-17 A) observed on MI355X for the tiled kernel (MEASURED_C below: 0.1275, at the smallest shape; 0 on every peaked
input, whose rows are one-hot to fp32 and whose outputs are therefore exact bf16 values of v).  Mean |err| of the tiled kernel over the
wavefront-per-query kernel on the same inputs, measured: 1.0000 at every shape (largest difference 1.0256e-04 against 1.0255e-04).

End-to-end bounds: 2 x the (max, mean) error measured on MI355X (MEASURED_E2E), never above the tiny fixture's bounds (decode 0.06 / 0.01,
encode 0.05 / 0.008: tests/test_gpu_parity.py::test_vae_tiny_golden) -- the decode maxima (0.028 .. 0.042, the tail of 12 288 / 49 152 pixels
of magnitude up to 2.5) end at the ceiling.  Measured with RQAMD_VAE_ATTN_VALU (wavefront-per-query kernel) for comparison: vae_map16
decode 0.0493 / 0.00497, encode 0.0094 / 0.00175; vae_map32 decode 0.0252 / 0.00436, encode 0.0090 / 0.00150; fp16 engine, vae_map16: decode
0.0046 / 0.00062, encode 0.0012 / 0.00022.  get_codes agrees with the reference on 99.61 % / 99.95 % / 99.90 % of the codes and on every code
with a clear margin.  The seeded networks give nearly flat attention; the peaked
stand-alone cases are what exercise the online softmax."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':                                  # the kernel A/B child (see _child): no conftest here
    for p in (ROOT, os.path.join(ROOT, 'rq-vae-transformer_amd'), os.path.join(ROOT, 'tests')):
        sys.path.insert(0, p)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import kernel_check as kc  # noqa: E402
import oracle  # noqa: E402
import vae_attn_cases as A  # noqa: E402
import vae_map_cases as V  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (B, T, C): two key and two query tiles; an odd tile count with 6 channel blocks over 4 wavefronts; the FFHQ shape, widest C; five
# tiles; the 32 x 32 latent; the longest loop (refused before this kernel)
SHAPES = [(3, 128, 64), (2, 192, 192), (2, 256, 512), (1, 320, 512), (1, 1024, 128), (1, 4096, 64)]
KINDS = ['flat', 'peaked']
# largest observed (err - 1/2 ulp) / (2^-17 A) of the tiled kernel on MI355X
MEASURED_C = {((3, 128, 64), 'flat'): 0.1275, ((2, 192, 192), 'flat'): 0.1231, ((2, 256, 512), 'flat'): 0.1120, ((1, 320, 512), 'flat'): 0.0936,
              ((1, 1024, 128), 'flat'): 0.0480, ((1, 4096, 64), 'flat'): 0.0269, 'peaked (every shape)': 0.0}
# ceilings (the tiny fixture's bounds) and the measured (max, mean) errors on MI355X: decode_code, encode, forward's output
CEIL_DEC, CEIL_ENC = (0.06, 0.01), (0.05, 0.008)
MEASURED_E2E = {'vae_map16': {'decode_code': (0.0383, 0.00496), 'encode': (0.0092, 0.00174), 'forward': (0.0424, 0.00513)},
                'vae_map32': {'decode_code': (0.0283, 0.00433), 'encode': (0.0088, 0.00150), 'forward': (0.0307, 0.00443)},
                'vae_map64': {'decode_code': (0.0388, 0.00452), 'encode': (0.0102, 0.00152), 'forward': (0.0420, 0.00455)}}


def _bound(name, what):
    ceil = CEIL_ENC if what == 'encode' else CEIL_DEC
    m = MEASURED_E2E.get(name, {}).get(what)
    return ceil if m is None else (min(ceil[0], 2 * m[0]), min(ceil[1], 2 * m[1]))


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    return _native


_CASES = {}


def _case(shape, kind):
    """(poisoned qkv view on the GPU, fp64 ref, A) -- computed once per (shape, kind), shared, never written to"""
    if (shape, kind) not in _CASES:
        B, T, C = shape
        qkv = A.make_qkv(B, T, C, kind, seed=1000 + T + C).to(DEV)
        ref, mag = A.reference(qkv)
        _CASES[(shape, kind)] = (kc.poisoned(qkv.view(B * T, 3 * C)).view(B, T, 3 * C), ref, mag)      # NaN rows behind the last token
    return _CASES[(shape, kind)]


def _launch(nat, qkv, form):
    """one launch into a NaN-guarded output; returns the output view after checking the guards"""
    B, T, C3 = qkv.shape
    buf, out = kc.guarded((B, T, C3 // 3), torch.bfloat16, qkv.device)
    nat.dbg_vae_attn(qkv, form=form, out=out)
    torch.cuda.synchronize()
    kc.check_guard(buf, out.numel(), f'vae attention form {form} {tuple(qkv.shape)}')
    return out


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_vae_attn_tiled_vs_fp64(nat, shape, kind):
    qkv, ref, mag = _case(shape, kind)
    out = _launch(nat, qkv, A.FORM_TILED)
    again = _launch(nat, qkv, A.FORM_TILED)
    assert torch.equal(_bits(out), _bits(again)), 'two launches on the same input differ'
    err = (out.double() - ref).abs()
    ratio_now = float(((err - 0.5 * kc.bf16_ulp(ref)).clamp_min(0.0) / (2.0 ** -17 * mag).clamp_min(1e-300)).max())
    print('vae attention tiled %s %s: observed c %.4f, mean |err| %.3e, max |err| %.3e' % (shape, kind, ratio_now, float(err.mean()), float(err.max())))
    A.check(out, ref, mag, what=f'tiled {shape} {kind}')
    # the launcher's own choice at these shapes is this kernel
    assert torch.equal(_bits(_launch(nat, qkv, A.FORM_AUTO)), _bits(out))


def test_vae_attn_tiled_mean_error_vs_wavefront_kernel(nat):
    """mean |err| of the tiled kernel <= 1.1 x that of the wavefront-per-query kernel (fp32 probabilities) on the same inputs, wherever the
    latter runs (T <= 1024): both are dominated by the same final bf16 rounding; a 16-bit P adds under 1 % in quadrature, a single bf16 P
    would add about 12 %.  Each mean is over >= 1e5 outputs: per (shape, kind) where the shape has that many, the two small shapes pooled."""
    pooled = {3: [0.0, 0], 1: [0.0, 0]}
    for shape in SHAPES:
        if shape[1] > 1024:
            continue
        for kind in KINDS:
            qkv, ref, mag = _case(shape, kind)
            s = {}
            for form in (A.FORM_WAVE, A.FORM_TILED):
                out = _launch(nat, qkv, form)
                if form == A.FORM_WAVE:
                    A.check(out, ref, mag, what=f'wavefront kernel {shape} {kind}')
                s[form] = float((out.double() - ref).abs().sum())
            n = ref.numel()
            print('vae attention %s %s: mean |err| tiled %.4e, wavefront-per-query %.4e, ratio %.4f (%d outputs)'
                  % (shape, kind, s[3] / n, s[1] / n, s[3] / max(s[1], 1e-300), n))
            if n >= 100000:
                assert s[3] <= 1.1 * s[1], (shape, kind)
            else:
                for form in (1, 3):
                    pooled[form][0] += s[form]
                    pooled[form][1] += n
    assert pooled[3][1] >= 100000
    print('vae attention small shapes pooled (%d outputs): ratio %.4f' % (pooled[3][1], pooled[3][0] / max(pooled[1][0], 1e-300)))
    assert pooled[3][0] <= 1.1 * pooled[1][0]


@pytest.mark.parametrize('shape', [(3, 128, 64), (3, 256, 512)], ids=lambda s: 'x'.join(map(str, s)))
def test_vae_attn_tiled_batch_invariance(nat, shape):
    """image 1 of a 3-image launch equals its own 1-image launch bit for bit"""
    B, T, C = shape
    qkv = A.make_qkv(B, T, C, 'flat', seed=5).to(DEV)
    three = _launch(nat, qkv, A.FORM_TILED)
    one = _launch(nat, qkv[1:2].contiguous(), A.FORM_TILED)
    assert torch.equal(_bits(three[1:2]), _bits(one))


def test_vae_attn_refusals(nat):
    def run(T, C, form=A.FORM_AUTO):
        return nat.dbg_vae_attn(torch.zeros((1, T, 3 * C), dtype=torch.bfloat16, device=DEV), form=form)
    with pytest.raises(NotImplementedError, match='4160 tokens > 4096'):
        run(4160, 64)
    with pytest.raises(NotImplementedError, match='1100 tokens > 1024'):
        run(1100, 64)
    with pytest.raises(NotImplementedError, match='tiled kernel needs'):
        run(4096, 576, A.FORM_TILED)
    with pytest.raises(NotImplementedError, match='1088 tokens > 1024'):
        run(1088, 64, A.FORM_WAVE)


# ------------------------------------------------------------------------------------------------ end to end
def _model(name):
    from rqvae.models.rqvae import RQVAE
    hps, dd = V.CASES[name][0]
    vae = RQVAE(**hps, ddconfig=dd, checkpointing=False)
    params = oracle.make_params(oracle.rqvae_param_shapes(hps, dd), V.SEED)
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return vae.to(DEV).eval()


def _errors(name):
    """every end-to-end figure of one fixture on the current engine: {what: (max err, mean err)}, code agreement, loss"""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))
    vae = _model(name)
    x = torch.from_numpy(g['x']).to(DEV)
    codes_ref = g['codes'].astype(np.int64)
    res = {}

    def pair(got, want):
        e = np.abs(got.detach().cpu().numpy().astype(np.float64) - want.astype(np.float64))
        return float(e.max()), float(e.mean())
    res['decode_code'] = pair(vae.decode_code(torch.from_numpy(codes_ref).to(DEV)), g['decode_code'])
    res['encode'] = pair(vae.encode(x), g['z_e'])
    codes = vae.get_codes(x).cpu().numpy()
    out, loss, fcodes = vae(x)
    assert np.array_equal(fcodes.cpu().numpy(), codes)
    same = codes == codes_ref
    # forward's pixels are decode(quantise(encode(x))), and every AttnBlock and GroupNorm spreads one latent over the whole image: where a code
    # with an unclear top-2 margin legitimately falls on the other side (2 of 512 in vae_map16), the stored pixels belong to another code map
    # (measured: mean 0.067, max 1.42 off).  Then the reference for forward's output is the fp32 oracle's decode of the codes forward itself
    # returned (oracle vs reference: below 5e-5 on these fixtures, make_golden_vae_maps.py); with every code equal it is the fixture.
    if same.all():
        want = g['forward_out']
    else:
        hps, dd = V.CASES[name][0]
        want = oracle.RQVAEOracle(hps, dd, oracle.make_params(oracle.rqvae_param_shapes(hps, dd), V.SEED)).decode_code(codes)
    res['forward'] = pair(out, want)
    # a code is owed where its own top-2 gap and that of every shallower depth is clear (a flipped code changes the residual below it)
    owed = np.cumprod(g['clear'], axis=-1).astype(bool)
    res['codes'] = (float(same.mean()), float(owed.mean()), int((~same & owed).sum()))
    res['loss'] = (float(loss), float(g['loss']))
    return res


def _check_e2e(name, res, tag):
    for what in ('decode_code', 'encode', 'forward'):
        print('%s %s %s: max err %.4f mean %.5f' % (name, tag, what, *res[what]))
    print('%s %s get_codes: agreement %.4f overall, %.4f of the codes clear, %d clear codes differ; loss %.5f (reference %.5f)'
          % ((name, tag) + res['codes'] + res['loss']))
    for what in ('decode_code', 'encode'):
        b = _bound(name, what)
        assert res[what][0] < b[0] and res[what][1] < b[1], (what, res[what], b)
    assert res['codes'][2] == 0, 'a code with a clear top-2 margin differs from the reference'
    b = _bound(name, 'forward')
    assert res['forward'][0] < b[0] and res['forward'][1] < b[1], (res['forward'], b)
    assert abs(res['loss'][0] - res['loss'][1]) < 0.05 * res['loss'][1] + 1e-3


@pytest.mark.parametrize('name', list(V.CASES))
def test_vae_map_golden(nat, name):
    """decode_code, encode, get_codes and forward of an RQ-VAE whose five AttnBlocks see 256 / 1024 / 4096 tokens, against the reference"""
    _check_e2e(name, _errors(name), 'bf16')


def test_vae_map16_fp16_engine(nat, monkeypatch):
    """the same through the fp16 build of the engine (RQAMD_VAE=fp16, librqamd_f16.so: the tiled kernel compiled with -DRQ_F16=1)"""
    monkeypatch.setenv('RQAMD_VAE', 'fp16')
    _check_e2e('vae_map16', _errors('vae_map16'), 'fp16')


def test_vae_map16_batches_chunks_and_read_ahead(nat, monkeypatch):
    """the 16 x 16 latent through the engine's batch machinery: rows of a 5-image call equal the one-image calls bit for bit; so do per-row
    calls on views of the batch (served from read-ahead windows) and an engine that works in chunks of two images (RQAMD_VAE_CHUNK=2:
    two-phase calls, the <= 16^2 layers -- every attention -- over a super-chunk, the rest chunk by chunk)"""
    hps = V.CASES['vae_map16'][0][0]
    rng = np.random.default_rng(9)
    codes = torch.from_numpy(rng.integers(0, hps['n_embed'], (5, 16, 16, 2))).to(DEV)
    x = torch.from_numpy(V.image(V.CASES['vae_map16'][0], seed=10, n_img=5)).to(DEV)
    vae = _model('vae_map16')
    dec, z_e = vae.decode_code(codes), vae.encode(x)
    for i in (0, 3, 4):
        assert torch.equal(vae.decode_code(codes[i:i + 1].clone()), dec[i:i + 1]), i
        assert torch.equal(vae.encode(x[i:i + 1].clone()), z_e[i:i + 1]), i
    rows = torch.cat([vae.decode_code(codes[i:i + 1]) for i in range(5)])
    assert torch.equal(rows, dec) and vae._ahead.hits > 0
    monkeypatch.setenv('RQAMD_VAE_CHUNK', '2')
    chunked = _model('vae_map16')
    assert torch.equal(chunked.decode_code(codes), dec)
    assert torch.equal(chunked.encode(x), z_e)


def _child(name):
    print('RESULT ' + json.dumps(_errors(name)))


@pytest.mark.parametrize('name', ['vae_map16', 'vae_map32'])
def test_vae_map_kernel_ab(nat, name):
    """RQAMD_VAE_ATTN_VALU (read once per process: a fresh child) sends the same attentions through the wavefront-per-query kernel; both
    engines meet the same bounds, printed side by side"""
    env = dict(os.environ, RQAMD_VAE_ATTN_VALU='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    valu = {k: tuple(v) for k, v in json.loads(line[len('RESULT '):]).items()}
    tiled = _errors(name)
    for what in ('decode_code', 'encode', 'forward'):
        print('%s %s (max, mean): tiled %.4f %.5f | wavefront-per-query %.4f %.5f' % ((name, what) + tiled[what] + valu[what]))
    _check_e2e(name, valu, 'RQAMD_VAE_ATTN_VALU')
    _check_e2e(name, tiled, 'tiled')


if __name__ == '__main__':
    _child(sys.argv[1])
