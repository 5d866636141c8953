"""ctypes binding of librqamd.so (include/rqamd.h) -- the only bridge between the Python mirror of the
reference's ``rqvae.models`` API and the gfx950 kernels.

There is no CPU path: if the library (or a GPU tensor) is missing this module raises.  PyTorch is used
for device memory and streams only; every argument crossing the ABI is a raw pointer / size."""
import contextlib
import math
import ctypes as C
import os

import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, 'librqamd.so')
# the two engines compiled once more with IEEE fp16 as their 16-bit storage type (csrc/rq_hip.h, -DRQ_F16=1; build.py): what
# RQTransformer.sample(amp=True) / forward(amp=True) and the opt-in RQAMD_VAE=fp16 RQ-VAE run on.  Same entry points, same ABI version;
# RqtEngine(half=True) / VaeEngine(half=True) bind to it.
LIB16_PATH = os.path.join(_PKG, 'librqamd_f16.so')

_lib = None
_lib16 = None
ABI_VERSION = 7
RQT_MAX_CONTEXT = 1088      # include/rqamd.h: RQAMD_RQT_MAX_CONTEXT, the longest body context (H * W + block_size_cond - 1) rqamd_rqt_create accepts


class RqamdError(RuntimeError):
    status = None


class RqamdOutOfMemory(RqamdError):
    """RQAMD_ERR_NOMEM: an engine workspace did not fit the free device memory"""
    status = -5


class VaeConfig(C.Structure):
    _fields_ = [('ch', C.c_int), ('out_ch', C.c_int), ('in_channels', C.c_int), ('resolution', C.c_int),
                ('z_channels', C.c_int), ('num_res_blocks', C.c_int), ('n_levels', C.c_int), ('ch_mult', C.c_int * 8),
                ('n_attn_res', C.c_int), ('attn_resolutions', C.c_int * 8), ('embed_dim', C.c_int), ('double_z', C.c_int)]


class RqtConfig(C.Structure):
    _fields_ = [('embed_dim', C.c_int), ('n_head', C.c_int), ('n_layer_body', C.c_int), ('n_layer_head', C.c_int),
                ('vocab_size', C.c_int), ('input_embed_dim', C.c_int), ('vocab_size_cond', C.c_int),
                ('block_size_cond', C.c_int), ('H', C.c_int), ('W', C.c_int), ('D', C.c_int), ('gelu_v2', C.c_int),
                ('input_emb_vqvae', C.c_int), ('head_emb_vqvae', C.c_int), ('shared_tok_emb', C.c_int), ('shared_cls_emb', C.c_int),
                ('cumsum_depth_ctx', C.c_int), ('vocab_sizes', C.c_int * 8)]


_SIGS = {
    'rqamd_abi_version': (C.c_int, []),
    'rqamd_last_error': (C.c_char_p, []),
    'rqamd_rq_quantize': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int64,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'rqamd_rq_code_norms': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_rq_soft_codes': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int64,
                                      C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_void_p]),
    'rqamd_rq_distances': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'rqamd_rq_ema_accumulate': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_rq_ema_update': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]),
    'rqamd_rq_ema_normalize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    'rqamd_rq_embed': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int64, C.c_int,
                                 C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_sample_logits': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64, C.c_uint64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_soft_ce': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_sample_logits_rows': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                           C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_sample_logits_logp': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    'rqamd_sample_logits_trunc': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float,
                                            C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_vae_create': (C.c_int, [C.POINTER(VaeConfig), C.POINTER(C.c_void_p)]),
    'rqamd_vae_destroy': (C.c_int, [C.c_void_p]),
    'rqamd_vae_set_option': (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    'rqamd_vae_set_param': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    'rqamd_vae_decode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_vae_encode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_create': (C.c_int, [C.POINTER(RqtConfig), C.POINTER(C.c_void_p)]),
    'rqamd_rqt_destroy': (C.c_int, [C.c_void_p]),
    'rqamd_rqt_set_option': (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    'rqamd_rqt_set_param': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    'rqamd_rqt_sample': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int,
                                   C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_uint64, C.c_uint64, C.c_int,
                                   C.c_void_p, C.c_void_p]),
    'rqamd_rqt_sample_masked': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
                                          C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_uint64, C.c_uint64, C.c_int,
                                          C.c_void_p, C.c_void_p]),
    'rqamd_rqt_sample_guided': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int),
                                          C.POINTER(C.c_float), C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_guide_logits': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_sample_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int),
                                        C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.c_uint64, C.c_uint64,
                                        C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_sample_logp': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_sample_trunc': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]),
    'rqamd_rqt_sample_schedule': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                            C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]),
    'rqamd_rqt_sample_shared': (C.c_int, [C.c_void_p, C.c_int]),
    'rqamd_rqt_sample_compose': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_compose_logits': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_sample_anchor': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    'rqamd_anchor_logits': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'rqamd_rqt_kv_bytes': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'rqamd_rqt_graph_captures': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'rqamd_rqt_logits': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    'rqamd_rqt_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_forward_onepass': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_log_probs': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_soft_loss': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_void_p), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_step_begin': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    'rqamd_rqt_step_prefill': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'rqamd_rqt_step_run': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'rqamd_rqt_step_logits': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    'rqamd_rqt_step_set_code': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_step_end': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_rqt_set_profile': (C.c_int, [C.c_void_p, C.c_int]),
    'rqamd_rqt_get_profile': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)]),
    'rqamd_rqt_get_profile_attn': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'rqamd_dbg_gemm_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'rqamd_dbg_conv_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'rqamd_dbg_conv_halo_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rqamd_dbg_set_row_scale': (C.c_int, [C.c_int]),
    'rqamd_dbg_rqt_share_params': (C.c_int, [C.c_void_p, C.c_void_p]),
    'rqamd_dbg_mfma_rate': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    'rqamd_dbg_conv_in_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_dbg_ups_subpixel_weights': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_dbg_conv_out_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p]),
    'rqamd_dbg_vae_attn': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_dbg_rqt_attn_decode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_dbg_rqt_attn_prefill': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_dbg_rqt_attn_extend': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p]),
    'rqamd_dbg_rqt_attn_packed': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'rqamd_dbg_rqt_attn_shared': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}
EXPORTS = tuple(_SIGS)


EXPORTS_F16 = tuple(n for n in _SIGS if n.startswith('rqamd_rqt_') or n.startswith('rqamd_vae_')) + ('rqamd_abi_version', 'rqamd_last_error', 'rqamd_dbg_set_row_scale',
                                                                                                           'rqamd_dbg_rqt_attn_decode', 'rqamd_dbg_rqt_attn_shared',
                                                                                                           'rqamd_dbg_rqt_attn_prefill', 'rqamd_dbg_rqt_attn_extend')


def _bind(path, names=None):
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        if names is not None and name not in names:
            continue
        fn = getattr(lib, name)           # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    if lib.rqamd_abi_version() != ABI_VERSION:
        raise RqamdError(f'{path}: ABI version {lib.rqamd_abi_version()} != {ABI_VERSION} (rebuild: python rq-vae-transformer_amd/build.py)')
    return lib


def lib():
    """The loaded librqamd.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RqamdError(f'{LIB_PATH} not found: build it with `python rq-vae-transformer_amd/build.py` '
                             '(hipcc --offload-arch=gfx950). There is no CPU fallback.')
        _lib = _bind(LIB_PATH)
    return _lib


def lib16():
    """librqamd_f16.so (the fp16 build of the RQ-Transformer engine); raises when it has not been built."""
    global _lib16
    if _lib16 is None:
        if not os.path.exists(LIB16_PATH):
            raise RqamdError(f'{LIB16_PATH} not found: build it with `python rq-vae-transformer_amd/build.py` '
                             '(hipcc --offload-arch=gfx950 -DRQ_F16=1). There is no CPU fallback.')
        _lib16 = _bind(LIB16_PATH, EXPORTS_F16)
    return _lib16


def kernel_source_hash(files=('gemm.h', 'gemm.hip')):
    """sha256[:16] over kernel sources under csrc/: stamps measurements that were taken out of run (PMC traffic files under
    profiles/) with the kernels they were taken on, so that bench.py can refuse a stale one."""
    import hashlib
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(_PKG, 'csrc', f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def check(status, L=None):
    if status != 0:
        msg = (L or lib()).rqamd_last_error().decode(errors='replace')
        if status == -1:
            raise ValueError(msg)
        if status == -2:
            raise NotImplementedError(msg)
        if status == -5:
            raise RqamdOutOfMemory(f'librqamd: out of device memory: {msg}')
        raise RqamdError(f'librqamd status {status}: {msg}')


def ptr(t, dtype=None):
    """Raw device pointer of a contiguous tensor (validated)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RqamdError('librqamd needs CUDA(HIP) tensors on an MI355X; got a CPU tensor (no CPU fallback exists)')
    if not t.is_contiguous():
        raise ValueError('non-contiguous tensor passed to librqamd')
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f'expected {dtype}, got {t.dtype}')
    return C.c_void_p(t.data_ptr())


def stream_of(t):
    if t.is_cuda:
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return C.c_void_p(0)


def on_device_of(t):
    """Context that makes t's device the current HIP device for the duration of a native call: the library allocates
    (engine workspaces, graphs) and sets kernel attributes on the CURRENT device, while the stream passed in belongs to
    the tensor's device -- model.to('cuda:1') with current device 0 must not mix the two."""
    dev = t if isinstance(t, torch.device) else t.device
    return torch.cuda.device(dev) if dev.type == 'cuda' else contextlib.nullcontext()


def _view_f32(address, shape, device):
    """A float32 tensor over `address` (device memory owned by the library; no copy, no ownership)."""
    n = 1
    for s_ in shape:
        n *= int(s_)

    class _Mem:
        __cuda_array_interface__ = {'shape': (n,), 'typestr': '<f4', 'data': (int(address), False), 'version': 2}
    with on_device_of(device):
        return torch.as_tensor(_Mem(), device=device).view(*shape)


def _ptr_array(tensors, dtype=torch.float32):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = ptr(t, dtype).value
    return arr


def _int_array(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])


# ---------------------------------------------------------------------------------------------- free functions
def rq_code_norms(codebook):
    """||c||^2 per code of a (K, dim) fp32 codebook (the codebook term of compute_distances)."""
    K, dim = codebook.shape
    out = torch.empty((K,), dtype=torch.float32, device=codebook.device)
    with on_device_of(codebook):
        check(lib().rqamd_rq_code_norms(ptr(codebook, torch.float32), K, dim, ptr(out), stream_of(codebook)))
    return out


def _out_like(out, shape, dtype, device, name):
    """the caller's output buffer (tests: a view into a guard-filled buffer) after a shape / dtype / device check, or a fresh one"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device:
        raise ValueError(f'{name}: out must be a {tuple(shape)} {dtype} tensor on {device}')
    return out


def rq_quantize(x, codebooks, want_quants=True, norms=None, out=None):
    """x (n_vec, dim) fp32; codebooks: list of (K_i, dim) fp32 (padding row excluded); norms: list of rq_code_norms(cb)
    (computed here when not given -- callers that quantise repeatedly cache them per codebook version); out: (codes, quant_cum)
    buffers to write into (quant_cum None when not want_quants).
    -> codes (n_vec, depth) int64, quant_cum (depth, n_vec, dim) fp32 or None."""
    n_vec, dim = x.shape
    depth = len(codebooks)
    for cb in codebooks:
        if cb.dim() != 2 or cb.shape[1] != dim:
            raise ValueError(f'codebook of shape {tuple(cb.shape)} does not match vectors of dim {dim}')
    if norms is None:
        norms, seen = [], {}
        for cb in codebooks:
            key = (cb.data_ptr(), cb.shape[0])
            if key not in seen:
                seen[key] = rq_code_norms(cb)
            norms.append(seen[key])
    out_codes, out_quants = out if out is not None else (None, None)
    codes = _out_like(out_codes, (n_vec, depth), torch.int64, x.device, 'rq_quantize codes')
    quants = _out_like(out_quants, (depth, n_vec, dim), torch.float32, x.device, 'rq_quantize quant_cum') if want_quants else None
    ws = None
    if 0 < n_vec < 96 * 64:          # small inputs: scratch for the codebook-split path (residual + per-split partial minima)
        ws = torch.empty((n_vec * dim * 4 + n_vec * 64 * 8,), dtype=torch.uint8, device=x.device)
    with on_device_of(x):
        check(lib().rqamd_rq_quantize(ptr(x, torch.float32), _ptr_array(codebooks), _ptr_array(norms),
                                      _int_array([c.shape[0] for c in codebooks]), depth, n_vec, dim, ptr(codes), ptr(quants),
                                      ptr(ws), 0 if ws is None else ws.numel(), stream_of(x)))
    return codes, quants


def rq_soft_codes(x, codebooks, norms, temp=1.0, stochastic=False, seed=0, offset=0, out=None):
    """x (n_vec, dim) fp32 -> (soft codes (n_vec, depth, K) fp32, codes (n_vec, depth) int64): RQBottleneck.get_soft_codes.
    out: (soft, codes) buffers to write into."""
    n_vec, dim = x.shape
    depth, K = len(codebooks), codebooks[0].shape[0]
    out_soft, out_codes = out if out is not None else (None, None)
    soft = _out_like(out_soft, (n_vec, depth, K), torch.float32, x.device, 'rq_soft_codes soft')
    codes = _out_like(out_codes, (n_vec, depth), torch.int64, x.device, 'rq_soft_codes codes')
    ws = torch.empty((max(n_vec, 1) * (dim * 4 + 512 + K * 4),), dtype=torch.uint8, device=x.device)
    with on_device_of(x):
        check(lib().rqamd_rq_soft_codes(ptr(x, torch.float32), _ptr_array(codebooks), _ptr_array(norms),
                                        _int_array([c.shape[0] for c in codebooks]), depth, n_vec, dim, float(temp), int(bool(stochastic)),
                                        int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), ptr(soft), ptr(codes), ptr(ws), ws.numel(),
                                        stream_of(x)))
    return soft, codes


def soft_ce(logits, targets, out=None):
    """soft_target_cross_entropy(logits, targets, reduction='none') (rqvae/optimizer/loss.py:68-84): logits, targets (rows, V) fp32 whose
    rows are contiguous (any row stride >= V: a column slice of a wider matrix is taken as it is) -> (rows,) fp32.  out: buffer to write into."""
    if logits.dim() != 2 or tuple(targets.shape) != tuple(logits.shape):
        raise ValueError(f'soft_ce: logits {tuple(logits.shape)} and targets {tuple(targets.shape)} must be two (rows, V) matrices of one shape')
    rows, V = logits.shape

    def rows_of(t):
        if t.dtype != torch.float32:
            raise ValueError(f'expected torch.float32, got {t.dtype}')
        if rows and V and (t.stride(1) != 1 or (rows > 1 and t.stride(0) < V)):
            t = t.contiguous()
        # (ptr() validates a contiguous tensor: pass the address of the first row and the row stride)
        return t, (t.stride(0) if rows > 1 else V)
    logits, ld = rows_of(logits)
    targets, ldt = rows_of(targets)
    out = _out_like(out, (rows,), torch.float32, logits.device, 'soft_ce')
    if rows == 0:
        return out
    if V < 1:
        raise ValueError('soft_ce: empty rows')
    with on_device_of(logits):
        check(lib().rqamd_soft_ce(ptr(logits.as_strided((1,), (1,)), torch.float32), ld, ptr(targets.as_strided((1,), (1,)), torch.float32), ldt,
                                  rows, V, ptr(out), stream_of(logits)))
    return out


def rq_distances(x, codebook, norms, out=None):
    """x (n_vec, dim) fp32, codebook (K, dim) fp32 -> (n_vec, K) fp32 squared distances ||x||^2 + ||c||^2 - 2 x.c:
    VQEmbedding.compute_distances (quantizations.py:43-62), the values the quantiser's argmin is taken over.  out: buffer to write into."""
    n_vec, dim = x.shape
    K = codebook.shape[0]
    out = _out_like(out, (n_vec, K), torch.float32, x.device, 'rq_distances')
    ws = torch.empty((max(n_vec, 1) * 512,), dtype=torch.uint8, device=x.device)
    with on_device_of(x):
        check(lib().rqamd_rq_distances(ptr(x, torch.float32), ptr(codebook, torch.float32), ptr(norms, torch.float32), K, n_vec, dim,
                                       ptr(out), ptr(ws), ws.numel(), stream_of(x)))
    return out


def rq_ema_accumulate(x, idx, n_embed):
    """x (n_vec, dim) fp32, idx (n_vec) int64 -> (count (n_embed,), sum (n_embed, dim)) fp32: VQEmbedding._update_buffers' one-hot sums."""
    n_vec, dim = x.shape
    count = torch.empty((n_embed,), dtype=torch.float32, device=x.device)
    vsum = torch.empty((n_embed, dim), dtype=torch.float32, device=x.device)
    with on_device_of(x):
        check(lib().rqamd_rq_ema_accumulate(ptr(x, torch.float32), ptr(idx, torch.int64), n_vec, dim, n_embed, ptr(count), ptr(vsum), stream_of(x)))
    return count, vsum


def rq_ema_update(cluster_size_ema, embed_ema, count, vsum, restart_vectors, decay):
    """in place: the EMA step of the codebook statistics + (restart_vectors given) the dead-code restart."""
    n_embed, dim = embed_ema.shape
    with on_device_of(embed_ema):
        check(lib().rqamd_rq_ema_update(ptr(cluster_size_ema, torch.float32), ptr(embed_ema, torch.float32), ptr(count, torch.float32),
                                        ptr(vsum, torch.float32), ptr(restart_vectors, torch.float32), n_embed, dim, float(decay),
                                        stream_of(embed_ema)))


def rq_ema_normalize(cluster_size_ema, embed_ema, n_total, eps, weight_out):
    """weight_out (n_embed, dim) <- embed_ema / normalised cluster size; n_total: device scalar = cluster_size_ema.sum()."""
    n_embed, dim = embed_ema.shape
    with on_device_of(embed_ema):
        check(lib().rqamd_rq_ema_normalize(ptr(cluster_size_ema, torch.float32), ptr(embed_ema, torch.float32), ptr(n_total, torch.float32),
                                           n_embed, dim, float(eps), ptr(weight_out, torch.float32), stream_of(embed_ema)))


def rq_embed(codes, codebooks, mode):
    """codes (n_vec, depth) int64 -> mode 0: (n_vec, dim); 1: (n_vec, depth, dim); 2: depth-cumsum."""
    n_vec, depth = codes.shape
    dim = codebooks[0].shape[1]
    shape = (n_vec, dim) if mode == 0 else (n_vec, depth, dim)
    out = torch.empty(shape, dtype=torch.float32, device=codes.device)
    with on_device_of(codes):
        check(lib().rqamd_rq_embed(ptr(codes, torch.int64), _ptr_array(codebooks), _int_array([c.shape[0] for c in codebooks]),
                                   depth, n_vec, dim, mode, ptr(out), stream_of(codes)))
    return out


def sample_logits(logits, temperature=1.0, top_k=None, top_p=None, seed=0, offset=0, want_probs=False, want_samples=True):
    rows, vocab = logits.shape
    samples = torch.empty((rows,), dtype=torch.int64, device=logits.device) if want_samples else None
    probs = torch.empty((rows, vocab), dtype=torch.float32, device=logits.device) if want_probs else None
    flags = torch.empty((max(rows, 1),), dtype=torch.int32, device=logits.device)
    with on_device_of(logits):
        check(lib().rqamd_sample_logits(ptr(logits, torch.float32), rows, vocab, float(temperature),
                                        0 if top_k is None else int(top_k), -1.0 if top_p is None else float(top_p),
                                        int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), ptr(samples), ptr(probs),
                                        ptr(flags), stream_of(logits)))
    return samples, probs


def sample_logits_rows(logits, temperature, top_k, top_p, seeds=None, seed=0, offset=0, want_probs=False, want_samples=True):
    """rqamd_sample_logits_rows: sample_logits with one temperature, top_k and top_p per row.  logits (rows, vocab) fp32; temperature
    (rows,) float32, top_k (rows,) int32 (<= 0 or >= vocab: off), top_p (rows,) float32 (< 0: off) and seeds (rows,) int64 or None are
    tensors on the device of `logits`.  Row r comes out as row r of sample_logits(logits, temperature[r], top_k[r], top_p[r], seed,
    offset); with seeds, as row 0 of sample_logits(logits[r:r+1], ..., seed=seeds[r], offset=0).  The values are not read on the host:
    the caller validates temperature > 0."""
    rows, vocab = logits.shape
    for name, t, dt in (('temperature', temperature, torch.float32), ('top_k', top_k, torch.int32), ('top_p', top_p, torch.float32),
                        ('seeds', seeds, torch.int64)):
        if t is None and name == 'seeds':
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != (rows,) or t.dtype != dt or t.device != logits.device:
            raise ValueError(f'sample_logits_rows: {name} must be a ({rows},) {dt} tensor on {logits.device}')
    samples = torch.empty((rows,), dtype=torch.int64, device=logits.device) if want_samples else None
    probs = torch.empty((rows, vocab), dtype=torch.float32, device=logits.device) if want_probs else None
    flags = torch.empty((max(rows, 1),), dtype=torch.int32, device=logits.device)
    with on_device_of(logits):
        check(lib().rqamd_sample_logits_rows(ptr(logits, torch.float32), rows, vocab, ptr(temperature), ptr(top_k), ptr(top_p), ptr(seeds),
                                             int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), ptr(samples), ptr(probs),
                                             ptr(flags), stream_of(logits)))
    return samples, probs


def sample_logits_logp(logits, logits_u=None, temperature=1.0, top_k=None, top_p=None, guidance_scale=1.0, row_temperature=None,
                       row_top_k=None, row_top_p=None, row_gscale=None, row_seeds=None, seed=0, offset=0, want_flags=True):
    """rqamd_sample_logits_logp: one draw per row and the log of its probability in the distribution it was drawn from.  logits (and
    logits_u, or None: unguided) (rows, vocab) fp32.  row_temperature None: the scalar form of sample_logits with temperature / top_k /
    top_p (/ guidance_scale); else the per-row form of sample_logits_rows with the device tensors row_temperature (rows,) float32,
    row_top_k (rows,) int32, row_top_p (rows,) float32 and, each or None, row_gscale (rows,) float32 and row_seeds (rows,) int64.
    want_flags False: no row_flags workspace (every filtered row takes the general kernel).  -> (samples (rows,) int64, draw (rows,) fp32)"""
    rows, vocab = logits.shape
    if logits_u is not None and tuple(logits_u.shape) != (rows, vocab):
        raise ValueError(f'sample_logits_logp: logits_u of shape {tuple(logits_u.shape)}; expected {(rows, vocab)}')
    for name, t, dt in (('row_temperature', row_temperature, torch.float32), ('row_top_k', row_top_k, torch.int32),
                        ('row_top_p', row_top_p, torch.float32), ('row_gscale', row_gscale, torch.float32), ('row_seeds', row_seeds, torch.int64)):
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != (rows,) or t.dtype != dt or t.device != logits.device):
            raise ValueError(f'sample_logits_logp: {name} must be a ({rows},) {dt} tensor on {logits.device}')
    samples = torch.empty((rows,), dtype=torch.int64, device=logits.device)
    draw = torch.empty((rows,), dtype=torch.float32, device=logits.device)
    flags = torch.empty((max(rows, 1),), dtype=torch.int32, device=logits.device) if want_flags else None
    with on_device_of(logits):
        check(lib().rqamd_sample_logits_logp(ptr(logits, torch.float32), ptr(logits_u, torch.float32), rows, vocab, float(temperature),
                                             0 if top_k is None else int(top_k), -1.0 if top_p is None else float(top_p),
                                             float(guidance_scale), ptr(row_temperature), ptr(row_top_k), ptr(row_top_p), ptr(row_gscale),
                                             ptr(row_seeds), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), ptr(samples), ptr(draw),
                                             ptr(flags), stream_of(logits)))
    return samples, draw


def sample_logits_trunc(logits, logits_u=None, temperature=1.0, top_k=None, top_p=None, min_p=None, typical_p=None, guidance_scale=1.0,
                        row_temperature=None, row_top_k=None, row_top_p=None, row_min_p=None, row_typical_p=None, row_gscale=None,
                        row_seeds=None, seed=0, offset=0, want_probs=False, want_logp=False, want_flags=True):
    """rqamd_sample_logits_trunc: sample_logits_logp with min-p and locally typical sampling after top-p (min_p / typical_p None: off),
    as scalars or -- with row_temperature -- as the device tensors row_min_p / row_typical_p (rows,) float32, each or None.
    -> (samples (rows,) int64, probs (rows, vocab) fp32 or None, draw (rows,) fp32 or None)"""
    rows, vocab = logits.shape
    if logits_u is not None and tuple(logits_u.shape) != (rows, vocab):
        raise ValueError(f'sample_logits_trunc: logits_u of shape {tuple(logits_u.shape)}; expected {(rows, vocab)}')
    for name, t, dt in (('row_temperature', row_temperature, torch.float32), ('row_top_k', row_top_k, torch.int32),
                        ('row_top_p', row_top_p, torch.float32), ('row_min_p', row_min_p, torch.float32),
                        ('row_typical_p', row_typical_p, torch.float32), ('row_gscale', row_gscale, torch.float32),
                        ('row_seeds', row_seeds, torch.int64)):
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != (rows,) or t.dtype != dt or t.device != logits.device):
            raise ValueError(f'sample_logits_trunc: {name} must be a ({rows},) {dt} tensor on {logits.device}')
    samples = torch.empty((rows,), dtype=torch.int64, device=logits.device)
    probs = torch.empty((rows, vocab), dtype=torch.float32, device=logits.device) if want_probs else None
    draw = torch.empty((rows,), dtype=torch.float32, device=logits.device) if want_logp else None
    flags = torch.empty((max(rows, 1),), dtype=torch.int32, device=logits.device) if want_flags else None
    with on_device_of(logits):
        check(lib().rqamd_sample_logits_trunc(ptr(logits, torch.float32), ptr(logits_u, torch.float32), rows, vocab, float(temperature),
                                              0 if top_k is None else int(top_k), -1.0 if top_p is None else float(top_p),
                                              0.0 if min_p is None else float(min_p), -1.0 if typical_p is None else float(typical_p),
                                              float(guidance_scale), ptr(row_temperature), ptr(row_top_k), ptr(row_top_p), ptr(row_min_p),
                                              ptr(row_typical_p), ptr(row_gscale), ptr(row_seeds), int(seed) & (2 ** 64 - 1),
                                              int(offset) & (2 ** 64 - 1), ptr(samples), ptr(probs), ptr(draw), ptr(flags), stream_of(logits)))
    return samples, probs, draw


def guide_logits(c, u, scale):
    """rqamd_guide_logits: classifier-free guidance on raw logits, g = c + (scale - 1) (c - u) with -inf of `c` kept (the device function
    the guided samplers apply inside the engine).  c, u (rows, vocab) fp32, contiguous, same shape -> g (rows, vocab) fp32."""
    if c.dim() != 2 or tuple(u.shape) != tuple(c.shape):
        raise ValueError(f'guide_logits: logits of shapes {tuple(c.shape)} and {tuple(u.shape)}; expected two equal (rows, vocab)')
    if not math.isfinite(float(scale)):
        raise ValueError(f'guide_logits: scale {scale} is not finite')
    rows, vocab = c.shape
    out = torch.empty_like(c)
    with on_device_of(c):
        check(lib().rqamd_guide_logits(ptr(c, torch.float32), ptr(u, torch.float32), rows, vocab, float(scale), ptr(out), stream_of(c)))
    return out


MAX_EXTRA_CONDS = 4            # RQAMD_RQT_MAX_EXTRA_CONDS


def compose_logits(c, u, extras, weights, scale):
    """rqamd_compose_logits: composed guidance on raw logits, guide(c', u', scale) with the K extra rows folded into the pair first (the
    device function the engine's fold applies; include/rqamd.h: rqamd_rqt_sample_compose).  c, u (rows, vocab) fp32; extras (K, rows,
    vocab) fp32; weights (K, rows) fp32, all on one device, 1 <= K <= MAX_EXTRA_CONDS -> (rows, vocab) fp32."""
    if c.dim() != 2 or tuple(u.shape) != tuple(c.shape):
        raise ValueError(f'compose_logits: logits of shapes {tuple(c.shape)} and {tuple(u.shape)}; expected two equal (rows, vocab)')
    rows, vocab = c.shape
    if extras.dim() != 3 or tuple(extras.shape[1:]) != (rows, vocab) or not 1 <= extras.shape[0] <= MAX_EXTRA_CONDS:
        raise ValueError(f'compose_logits: extra logits of shape {tuple(extras.shape)}; expected (1 .. {MAX_EXTRA_CONDS}, {rows}, {vocab})')
    K = extras.shape[0]
    if tuple(weights.shape) != (K, rows):
        raise ValueError(f'compose_logits: weights of shape {tuple(weights.shape)}; expected ({K}, {rows})')
    if not math.isfinite(float(scale)):
        raise ValueError(f'compose_logits: scale {scale} is not finite')
    out = torch.empty_like(c)
    c, u, extras, weights = (t.contiguous() for t in (c, u, extras, weights))
    with on_device_of(c):
        check(lib().rqamd_compose_logits(ptr(c, torch.float32), ptr(u, torch.float32), ptr(extras, torch.float32), K, ptr(weights, torch.float32),
                                         rows, vocab, float(scale), ptr(out), stream_of(c)))
    return out


ANCHOR_DIMS = (64, 128, 192, 256)


def anchor_logits(logits, z_rows, codes, codebooks, norms, weight, logits_u=None, want_resid=False, want_dist=False):
    """rqamd_anchor_logits: the three stages of ONE anchored sampling step over given rows (include/rqamd.h: rqamd_rqt_sample_anchor) --
    the residual r = z_rows - codebooks[0][codes[:, 0]] - ... of depth d = codes.shape[1] in the quantiser's order and bits, its distances
    to codebooks[d] (the values of rq_distances), and logits - weight * dist through the device function of the engine's fold.
    logits (rows, vocab) fp32; z_rows (rows, dim) fp32; codes (rows, d) int64 (d = 0: depth 0; None is (rows, 0)); codebooks / norms:
    at least d + 1 tensors (vocab, dim) / (vocab,); weight (rows,) fp32 on the device; logits_u: the unconditional twins or None.
    -> out, or (out, out_u) with logits_u; want_resid / want_dist append the (rows, dim) residual / the (rows, vocab) distances."""
    if logits.dim() != 2 or (logits_u is not None and tuple(logits_u.shape) != tuple(logits.shape)):
        raise ValueError(f'anchor_logits: logits of shape {tuple(logits.shape)}' + ('' if logits_u is None else f' and {tuple(logits_u.shape)}')
                         + '; expected (rows, vocab)')
    rows, vocab = logits.shape
    if z_rows.dim() != 2 or z_rows.shape[0] != rows:
        raise ValueError(f'anchor_logits: z_rows of shape {tuple(z_rows.shape)}; expected ({rows}, dim)')
    dim = z_rows.shape[1]
    if dim not in ANCHOR_DIMS:
        raise NotImplementedError(f'anchor_logits: dim {dim} must be 64, 128, 192 or 256')
    d = 0 if codes is None else codes.shape[-1]
    if codes is not None and (codes.dim() != 2 or codes.shape[0] != rows):
        raise ValueError(f'anchor_logits: codes of shape {tuple(codes.shape)}; expected ({rows}, d)')
    if len(codebooks) <= d or len(norms) <= d:
        raise ValueError(f'anchor_logits: {len(codebooks)} codebooks / {len(norms)} norms for depth {d}')
    for cb, cn in zip(codebooks[:d + 1], norms[:d + 1]):
        if tuple(cb.shape) != (vocab, dim) or tuple(cn.shape) != (vocab,):
            raise ValueError(f'anchor_logits: codebook of shape {tuple(cb.shape)} with norms {tuple(cn.shape)}; expected ({vocab}, {dim}) and ({vocab},)')
    if tuple(weight.shape) != (rows,):
        raise ValueError(f'anchor_logits: weight of shape {tuple(weight.shape)}; expected ({rows},)')
    logits, z_rows, weight = logits.contiguous(), z_rows.contiguous(), weight.contiguous()
    logits_u = None if logits_u is None else logits_u.contiguous()
    codes = None if d == 0 else codes.to(torch.long).contiguous()
    out = torch.empty_like(logits)
    out_u = None if logits_u is None else torch.empty_like(logits)
    resid = torch.empty((rows, dim), dtype=torch.float32, device=logits.device) if want_resid else None
    dist = torch.empty((rows, vocab), dtype=torch.float32, device=logits.device) if want_dist else None
    if rows == 0:
        res = (out,) if logits_u is None else (out, out_u)
        res += ((resid,) if want_resid else ()) + ((dist,) if want_dist else ())
        return res[0] if len(res) == 1 else res
    ws = torch.empty((rows * 512 + 256 + rows * dim * 4 + 256 + rows * vocab * 4,), dtype=torch.uint8, device=logits.device)
    cbs, nrm = _ptr_array(list(codebooks[:d + 1])), _ptr_array(list(norms[:d + 1]))
    with on_device_of(logits):
        check(lib().rqamd_anchor_logits(ptr(logits, torch.float32), ptr(logits_u, torch.float32), ptr(z_rows, torch.float32), ptr(codes, torch.int64),
                                        cbs, nrm, d, dim, vocab, ptr(weight, torch.float32), rows, ptr(out), ptr(out_u), ptr(resid), ptr(dist),
                                        ptr(ws), ws.numel(), stream_of(logits)))
    res = (out,) if logits_u is None else (out, out_u)
    res += ((resid,) if want_resid else ()) + ((dist,) if want_dist else ())
    return res[0] if len(res) == 1 else res


def dbg_gemm(a_bf16, w_bf16, bias=None, epi=3, bm=0, bn=0, splitk=0, out=None):
    """diagnostics: out[M,N] = a[M,K] @ w[N,K]^T (+bias); a, w are torch.bfloat16."""
    M, K = a_bf16.shape
    N = w_bf16.shape[0]
    if out is None:
        kind = epi % 16                      # + 16 / + 64 / + 96 / ... are launch options (include/rqamd.h)
        if kind == 4:
            out = torch.empty((splitk if splitk > 0 else 8, M, N), dtype=torch.float32, device=a_bf16.device)
        else:
            out = torch.empty((M, N), dtype=torch.float32 if kind == 3 else torch.bfloat16, device=a_bf16.device)
    check(lib().rqamd_dbg_gemm_bf16(ptr(a_bf16, torch.bfloat16), ptr(w_bf16, torch.bfloat16), M, N, K, ptr(bias), epi,
                                    ptr(out), bm, bn, splitk, stream_of(a_bf16)))
    return out


def dbg_conv(x, w, bias=None, resid=None, ksize=3, stride=1, ups=0, bm=0, bn=0, flags=0, out=None):
    """diagnostics: x (B,Hs,Ws,Cin) bf16 NHWC, w (Cout,k,k,Cin) bf16 -> (B,Ho,Wo,Cout) bf16."""
    B, Hs, Ws, Cin = x.shape
    H, W = Hs << ups, Ws << ups
    Cout = w.shape[0]
    Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.bfloat16, device=x.device)
    check(lib().rqamd_dbg_conv_bf16(ptr(x, torch.bfloat16), ptr(w, torch.bfloat16), ptr(bias), ptr(resid), B, H, W, Cin, Cout,
                                    ksize, stride, ups, ptr(out), bm, bn, flags, stream_of(x)))
    return out


def dbg_ups_subpixel_weights(w):
    """diagnostics: (Cout,3,3,Cin) bf16 conv weights -> (4,Cout,2,2,Cin) bf16 pre-summed weights of the sub-pixel form of Upsample.conv."""
    Cout, _, _, Cin = w.shape
    wsub = torch.empty((4, Cout, 2, 2, Cin), dtype=torch.bfloat16, device=w.device)
    check(lib().rqamd_dbg_ups_subpixel_weights(ptr(w, torch.bfloat16), Cout, Cin, ptr(wsub), stream_of(w)))
    return wsub


def dbg_conv_halo(x, w, bias, gn=None, resid=None, out=None, stats=None, ups=False, persistent=None, wpx=0, subpixel=False):
    """diagnostics: halo-reuse 3x3 conv; x (B,H,W,Cin) bf16 (or (B,H/2,W/2,Cin) with ups), w (Cout,3,3,Cin) bf16, gn
    (B,Cin,2) fp32 or None; stats (B, (H/8)*(W/32), 32, 2) fp32 receives the per-tile GroupNorm partial sums.
    persistent True / False forces the persistent / per-tile form of the kernel (None: the default), wpx the persistent form's
    workgroups per XCD (0: one per CU)."""
    B, H, W, Cin = x.shape
    if ups:
        H, W = 2 * H, 2 * W
    Cout = w.shape[0]
    if out is None:
        out = torch.empty((B, H, W, Cout), dtype=torch.bfloat16, device=x.device)
    if subpixel:          # the upsample conv as four 2 x 2 convs over the source image (conv_halo.hip, UPS = 2)
        assert ups
        w = dbg_ups_subpixel_weights(w)
    check(lib().rqamd_dbg_conv_halo_bf16(ptr(x, torch.bfloat16), ptr(w, torch.bfloat16), ptr(bias, torch.float32), ptr(gn), ptr(resid),
                                         B, H, W, Cin, Cout,
                                         (1 if ups else 0) | (0 if persistent is None else 16 if persistent else 32) | ((int(wpx) & 0xff) << 8)
                                         | (64 if subpixel else 0),
                                         ptr(out), ptr(stats), stream_of(x)))
    return out


def dbg_mfma_rate(mode=1, n_per_wave=1 << 15, launches=64, secs=1.5, device='cuda'):
    """diagnostics: the dense bf16 MFMA rate (TFLOP/s) the board sustains with MFMAs alone -- mode 0 constant operands (the instruction
    rate), mode 1 operands that change every instruction (~N(0,1) bf16).  Runs for about `secs` seconds so that the clock settles under the
    power limit, and times the last batch of launches with events."""
    scratch = torch.zeros(16, dtype=torch.float32, device=device)
    flop = C.c_double(0.0)
    st = torch.cuda.current_stream(scratch.device)

    def batch():
        check(lib().rqamd_dbg_mfma_rate(int(mode), int(n_per_wave), int(launches), ptr(scratch), C.byref(flop), stream_of(scratch)))
    batch()
    torch.cuda.synchronize()
    import time
    t0, rate = time.time(), 0.0
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        batch()
        e1.record(st)
        e1.synchronize()
        rate = flop.value / (e0.elapsed_time(e1) * 1e-3) / 1e12
        if time.time() - t0 >= secs:
            return rate


def dbg_set_row_scale(factor):
    """diagnostics: variant selection sees rows * factor (1 = normal)."""
    check(lib().rqamd_dbg_set_row_scale(int(factor)))


def dbg_conv_in(x, w, bias):
    """diagnostics: MFMA conv_in; x (B,3,H,W) fp32, w (3,3,3,128) fp32 = (ky,kx,ci,cout), returns (B,H,W,128) bf16."""
    B, _, H, W = x.shape
    y = torch.empty((B, H, W, 128), dtype=torch.bfloat16, device=x.device)
    check(lib().rqamd_dbg_conv_in_bf16(ptr(x, torch.float32), ptr(w, torch.float32), ptr(bias, torch.float32), B, H, W, ptr(y),
                                       stream_of(x)))
    return y


def dbg_conv_out(x, w, bias, gn=None):
    """diagnostics: MFMA conv_out; x (B,H,W,Cin) bf16, w (Cout,3,3,Cin) fp32, returns (B,Cout,H,W) fp32."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    y = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    check(lib().rqamd_dbg_conv_out_bf16(ptr(x, torch.bfloat16), ptr(w, torch.float32), ptr(bias, torch.float32), ptr(gn),
                                        B, H, W, Cin, Cout, ptr(y), stream_of(x)))
    return y


def dbg_vae_attn(qkv, form=0, out=None):
    """diagnostics: AttnBlock's attention alone; qkv (B, T, 3C) bf16 -> (B, T, C) bf16 = softmax(q k^T C^-0.5) v per image.  form 0: the
    engine's choice, 1 the wavefront-per-query kernel, 2 the 64-token MFMA kernel, 3 the tiled MFMA kernel (NotImplementedError for a
    shape the form does not serve)."""
    B, T, C3 = qkv.shape
    if C3 % 3 != 0:
        raise ValueError(f'qkv of shape {tuple(qkv.shape)}: last dimension is not 3 C')
    if out is None:
        out = torch.empty((B, T, C3 // 3), dtype=torch.bfloat16, device=qkv.device)
    with on_device_of(qkv):
        check(lib().rqamd_dbg_vae_attn(ptr(qkv, torch.bfloat16), B, T, C3 // 3, int(form), ptr(out, torch.bfloat16), stream_of(qkv)))
    return out


def dbg_rqt_attn_decode(qkv, kc, vc, y, nh, Tcap, t, t_max=-1, ksc=None, vsc=None, step=None, step_base=0, half=False):
    """diagnostics: one decode step of the RQ-Transformer's attention alone (include/rqamd.h: rqamd_dbg_rqt_attn_decode).  qkv (rows, 3E)
    bf16, y (rows, E) bf16, caches (rows, nh, Tcap, hd) bf16 -- or uint8 with fp32 scales ksc / vsc (rows, nh, Tcap); step: a one-element
    int32 tensor through which t reaches the kernel (set to step_base first), or None.  half: the fp16 build of the library, every 16-bit
    tensor torch.float16."""
    rows, E3 = qkv.shape
    L, dt = (lib16(), torch.float16) if half else (lib(), torch.bfloat16)
    with on_device_of(qkv):
        check(L.rqamd_dbg_rqt_attn_decode(ptr(qkv, dt), ptr(kc), ptr(vc), ptr(ksc, torch.float32), ptr(vsc, torch.float32),
                                          rows, int(nh), E3 // 3, int(Tcap), int(t), int(t_max), ptr(step, torch.int32), int(step_base),
                                          ptr(y, dt), stream_of(qkv)), L)
    return y


def dbg_rqt_attn_shared(qkv, kcs, vcs, kc, vc, y, fan, nh, t, t_max=-1, step=None, step_base=0, half=False):
    """diagnostics: one decode step of the shared-prompt attention alone (include/rqamd.h: rqamd_dbg_rqt_attn_shared).  qkv (rows, 3E), y
    (rows, E), the group caches kcs / vcs (rows / fan, nh, Ps, 64) and the own caches kc / vc (rows, nh, Tcap_row, 64), bf16 -- or, half,
    torch.float16 through the fp16 build of the library; t: the global index of this token's key (Ps .. Ps + Tcap_row - 1); step as in
    dbg_rqt_attn_decode."""
    rows, E3 = qkv.shape
    L, dt = (lib16(), torch.float16) if half else (lib(), torch.bfloat16)
    Ps = int(kcs.shape[2]) if kcs is not None else 0
    Tcap = int(kc.shape[2]) if kc is not None else 0
    with on_device_of(qkv):
        check(L.rqamd_dbg_rqt_attn_shared(ptr(qkv, dt), ptr(kcs, dt), ptr(vcs, dt), ptr(kc, dt), ptr(vc, dt), rows, int(fan), int(nh), E3 // 3,
                                          Ps, Tcap, int(t), int(t_max), ptr(step, torch.int32), int(step_base), ptr(y, dt),
                                          stream_of(qkv)), L)
    return y


def dbg_rqt_attn_prefill(qkv, y, n_img, P, nh, Tcap, kc=None, vc=None, ksc=None, vsc=None, half=False):
    """diagnostics: the causal prefix attention alone (rqamd_dbg_rqt_attn_prefill).  qkv (n_img * P, 3E) bf16, y (n_img * P, E) bf16,
    caches as dbg_rqt_attn_decode with rows = n_img, or none at all (the cache-free form).  half: the fp16 build, as there."""
    L, dt = (lib16(), torch.float16) if half else (lib(), torch.bfloat16)
    with on_device_of(qkv):
        check(L.rqamd_dbg_rqt_attn_prefill(ptr(qkv, dt), ptr(kc), ptr(vc), ptr(ksc, torch.float32), ptr(vsc, torch.float32),
                                           int(n_img), int(P), int(nh), qkv.shape[-1] // 3, int(Tcap), ptr(y, dt),
                                           stream_of(qkv)), L)
    return y


def dbg_rqt_attn_extend(qkv, kc, vc, y, n_img, R, T0, nh, Tcap, half=False):
    """diagnostics: the cache-extending causal attention alone (rqamd_dbg_rqt_attn_extend, csrc/rqt_attn_extend.hip).  qkv (n_img * R, 3E)
    and y (n_img * R, E) bf16, caches (n_img, nh, Tcap, 64) bf16 holding rows 0 .. T0-1 -- or, half, torch.float16 through the fp16 build.
    Query r attends over cache rows < T0 and own keys 0 .. r; token r is appended at cache row T0 + r."""
    L, dt = (lib16(), torch.float16) if half else (lib(), torch.bfloat16)
    dev_t = qkv if qkv is not None else y
    with on_device_of(dev_t):
        check(L.rqamd_dbg_rqt_attn_extend(ptr(qkv, dt), ptr(kc, dt), ptr(vc, dt), int(n_img), int(R), int(T0), int(nh),
                                          (qkv.shape[-1] // 3) if qkv is not None else y.shape[-1], int(Tcap), ptr(y, dt), stream_of(dev_t)), L)
    return y


def dbg_rqt_attn_packed(qkv, y, group, nh):
    """diagnostics: causal attention inside groups of `group` <= 8 consecutive rows (rqamd_dbg_rqt_attn_packed).  qkv (rows, 3E) bf16,
    y (rows, E) bf16."""
    rows, E3 = qkv.shape
    with on_device_of(qkv):
        check(lib().rqamd_dbg_rqt_attn_packed(ptr(qkv, torch.bfloat16), rows, int(group), int(nh), E3 // 3, ptr(y, torch.bfloat16),
                                              stream_of(qkv)))
    return y


# ---------------------------------------------------------------------------------------------- engines
class _Engine:
    """Opaque native handle bound to ONE device: created, fed and run with that device current (on_device_of)."""
    _create = _destroy = _set = None

    def __init__(self, cfg_struct, device, half=False):
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self._h = C.c_void_p()
        self.half = bool(half)
        self._L = lib16() if half else lib()         # the library this handle belongs to (errors are per library, too)
        with on_device_of(self.device):
            check(getattr(self._L, self._create)(C.byref(cfg_struct), C.byref(self._h)), self._L)

    def _on_my_device(self, *tensors):
        for t in tensors:
            if t is not None and t.device != self.device:
                raise ValueError(f'tensor on {t.device}, engine on {self.device} (move the model and its inputs to one device)')

    def set_param(self, name, tensor):
        t = tensor.detach()
        self._on_my_device(t)
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        with on_device_of(self.device):
            check(getattr(self._L, self._set)(self._h, name.encode(), ptr(t, torch.float32), shape, t.dim(), stream_of(t)), self._L)
        if t.is_cuda:
            t.record_stream(torch.cuda.current_stream(t.device))

    def _run(self, fn):
        """One native call on the engine's device.  The engines allocate their workspaces with hipMalloc, outside torch's
        caching allocator: on an out-of-memory failure (RQAMD_ERR_NOMEM only -- any other error is raised as it is) the
        allocator's cached blocks are released and the call is retried once; the handle is left empty, not dangling, by a
        failed regrowth, and the library clears HIP's sticky last-error after the failed hipMalloc."""
        with on_device_of(self.device):
            try:
                return check(fn(), self._L)
            except RqamdOutOfMemory:
                if self.device.type != 'cuda':
                    raise
                torch.cuda.empty_cache()
                return check(fn(), self._L)

    def close(self):
        if self._h is not None and self._h.value and self._L is not None:
            getattr(self._L, self._destroy)(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VaeEngine(_Engine):
    _create, _destroy, _set = 'rqamd_vae_create', 'rqamd_vae_destroy', 'rqamd_vae_set_param'

    def __init__(self, ddconfig, embed_dim, device='cuda', half=False):
        c = VaeConfig()
        c.ch, c.out_ch, c.in_channels = ddconfig['ch'], ddconfig['out_ch'], ddconfig['in_channels']
        c.resolution, c.z_channels, c.num_res_blocks = ddconfig['resolution'], ddconfig['z_channels'], ddconfig['num_res_blocks']
        mult, attn = list(ddconfig['ch_mult']), list(ddconfig['attn_resolutions'])
        if len(mult) > 8 or len(attn) > 8:
            raise NotImplementedError('more than 8 resolution levels')
        c.n_levels, c.n_attn_res = len(mult), len(attn)
        for i, m in enumerate(mult):
            c.ch_mult[i] = int(m)
        for i, a in enumerate(attn):
            c.attn_resolutions[i] = int(a)
        c.embed_dim, c.double_z = int(embed_dim), int(bool(ddconfig.get('double_z', True)))
        self.cfg = c
        super().__init__(c, device, half=half)      # half: the fp16 build of the engine (opt-in RQAMD_VAE=fp16, see models/rqvae/rqvae.py)
        if not ddconfig.get('resamp_with_conv', True):      # bare nearest upsample / average pool (layers.py:20-57; no released config)
            check(self._L.rqamd_vae_set_option(self._h, b'resamp_with_conv', 0), self._L)

    def decode(self, z_q):
        """z_q (B,h,w,embed_dim) fp32 NHWC -> (B,out_ch,H,W) fp32"""
        c = self.cfg
        lr = c.resolution >> (c.n_levels - 1)
        if z_q.dim() != 4 or tuple(z_q.shape[1:]) != (lr, lr, c.embed_dim):
            # the engine is built for one resolution (its workspaces and tile schedules are sized from ddconfig.resolution)
            raise ValueError(f'decode: latent of shape {tuple(z_q.shape)}; this RQVAE decodes (B, {lr}, {lr}, {c.embed_dim})')
        self._on_my_device(z_q)
        B = z_q.shape[0]
        out = torch.empty((B, c.out_ch, c.resolution, c.resolution), dtype=torch.float32, device=z_q.device)
        self._run(lambda: self._L.rqamd_vae_decode(self._h, ptr(z_q, torch.float32), B, ptr(out), stream_of(z_q)))
        return out

    def encode(self, x):
        """x (B,in_channels,H,W) fp32 -> z_e (B,h,w,embed_dim) fp32 NHWC"""
        c = self.cfg
        if x.dim() != 4 or tuple(x.shape[1:]) != (c.in_channels, c.resolution, c.resolution):
            raise ValueError(f'encode: input of shape {tuple(x.shape)}; this RQVAE encodes (B, {c.in_channels}, {c.resolution}, {c.resolution})')
        self._on_my_device(x)
        B = x.shape[0]
        lr = c.resolution >> (c.n_levels - 1)
        out = torch.empty((B, lr, lr, c.embed_dim), dtype=torch.float32, device=x.device)
        self._run(lambda: self._L.rqamd_vae_encode(self._h, ptr(x, torch.float32), B, ptr(out), stream_of(x)))
        return out


class RqtEngine(_Engine):
    _create, _destroy, _set = 'rqamd_rqt_create', 'rqamd_rqt_destroy', 'rqamd_rqt_set_param'

    def __init__(self, *, embed_dim, n_head, n_layer_body, n_layer_head, vocab_size, input_embed_dim, vocab_size_cond,
                 block_size_cond, block_size, gelu_v2=False, device='cuda', input_emb_vqvae=True, head_emb_vqvae=True,
                 shared_tok_emb=True, shared_cls_emb=True, cumsum_depth_ctx=True, vocab_sizes=None, half=False, n_head_head=None):
        c = RqtConfig(embed_dim, n_head, n_layer_body, n_layer_head, vocab_size, input_embed_dim, vocab_size_cond,
                      block_size_cond, block_size[0], block_size[1], block_size[2], int(gelu_v2), int(bool(input_emb_vqvae)),
                      int(bool(head_emb_vqvae)), int(bool(shared_tok_emb)), int(bool(shared_cls_emb)), int(bool(cumsum_depth_ctx)))
        vs = list(vocab_sizes) if vocab_sizes is not None else [vocab_size] * block_size[2]
        for i, v in enumerate(vs[:8]):
            c.vocab_sizes[i] = int(v)
        self.cfg = c
        super().__init__(c, device, half=half)
        if n_head_head is not None and int(n_head_head) != int(n_head):       # head.block.n_head != body.block.n_head (no released config)
            check(self._L.rqamd_rqt_set_option(self._h, b'head.n_head', int(n_head_head)), self._L)

    def _check(self, codes, cond, codebooks):
        c = self.cfg
        if codes.dim() != 4 or tuple(codes.shape[1:]) != (c.H, c.W, c.D):
            raise ValueError(f'codes of shape {tuple(codes.shape)}; expected (B, {c.H}, {c.W}, {c.D})')
        n_cond = self._cond_rows(codes.shape[0])
        if cond is not None and tuple(cond.shape) != (n_cond, max(c.block_size_cond, 1)):
            raise ValueError(f'cond of shape {tuple(cond.shape)}; expected ({n_cond}, {max(c.block_size_cond, 1)})')
        if len(codebooks) < c.D:
            raise ValueError(f'{len(codebooks)} codebooks for depth {c.D}')
        if c.input_emb_vqvae or c.head_emb_vqvae:
            for d, cb in enumerate(codebooks[:c.D]):
                if cb.dim() != 2 or cb.shape[0] < c.vocab_sizes[d] or cb.shape[1] != c.input_embed_dim:
                    raise ValueError(f'codebook of shape {tuple(cb.shape)}; expected (>= {c.vocab_sizes[d]}, {c.input_embed_dim})')
        self._on_my_device(codes, cond, *codebooks[:c.D])

    def arm_shared(self, fan):
        """rqamd_rqt_sample_shared for the NEXT sample / sample_masked / sample_guided / sample_rows call of this object: a shared-prompt
        call of `fan` rows per group -- `partial` has G * fan rows, `cond` / `uncond` G rows.  0 / None disarms."""
        self._shared = int(fan) if fan else 0

    def _cond_rows(self, B):
        """rows of cond / uncond the next sampling call expects for B images"""
        fan = getattr(self, '_shared', 0)
        if not fan:
            return B
        if fan < 0 or B % fan:
            self._shared = 0
            raise ValueError(f'shared-prompt call: {B} images are not a multiple of the group size {fan}')
        return B // fan

    def arm_compose(self, conds=None, weights=None):
        """rqamd_rqt_sample_compose for the NEXT sample_guided / guided sample_rows call of this object: composed guidance.  `conds`: K
        tensors (B, block_size_cond) int64 on the engine's device, or None entries (zeros); `weights`: K * B finite floats on the host,
        condition-major.  None / an empty list disarms.  Checked when the call is made, before the library is called."""
        self._compose = (list(conds), [float(w) for w in weights]) if conds else None

    def _compose_arrays(self, B):
        """the arming of arm_compose as the arguments of rqamd_rqt_sample_compose, checked (ValueError), and consumed"""
        comp, self._compose = getattr(self, '_compose', None), None
        if comp is None:
            return None
        conds, w = comp
        K = len(conds)
        if K > MAX_EXTRA_CONDS:
            raise ValueError(f'{K} extra conditions; at most {MAX_EXTRA_CONDS}')
        if len(w) != K * B:
            raise ValueError(f'{len(w)} weights for {K} extra conditions of {B} images; expected {K * B}')
        if not all(math.isfinite(x) for x in w):
            raise ValueError('extra-condition weights must be finite')
        want = (B, max(self.cfg.block_size_cond, 1))
        for t in conds:
            if t is not None and tuple(t.shape) != want:
                raise ValueError(f'extra cond of shape {tuple(t.shape)}; expected {want}')
        self._on_my_device(*conds)
        parr = (C.c_void_p * K)()
        for i, t in enumerate(conds):
            parr[i] = None if t is None else ptr(t, torch.int64).value
        return K, parr, (C.c_float * (K * B))(*w), conds

    def arm_anchor(self, z=None, codebooks=None, norms=None, weight=None, per_image=False):
        """rqamd_rqt_sample_anchor for the NEXT sample / sample_masked / sample_guided / sample_rows call of this object: anchored sampling.
        `z` (B, H, W, dim) fp32 on the engine's device; `codebooks` / `norms`: D tensors (vocab_size, dim) / (vocab_size,) each; `weight`:
        a flat host sequence or tensor of H * W * D values >= 0 (per_image: B * H * W * D, image-major, depth last).  z None disarms.
        Checked when the call is made, before the library is called."""
        self._anchor = None if z is None else (z, list(codebooks), list(norms), weight, bool(per_image))

    def _anchor_arrays(self, B):
        """the arming of arm_anchor as the arguments of rqamd_rqt_sample_anchor, checked (ValueError / NotImplementedError), and consumed"""
        anc, self._anchor = getattr(self, '_anchor', None), None
        if anc is None:
            return None
        z, cbs, norms, weight, per_image = anc
        c = self.cfg
        if z.dim() != 4 or tuple(z.shape[:3]) != (B, c.H, c.W) or z.dtype != torch.float32:
            raise ValueError(f'anchor: z of shape {tuple(z.shape)} / {z.dtype}; expected ({B}, {c.H}, {c.W}, dim) / torch.float32')
        dim = z.shape[3]
        if dim not in ANCHOR_DIMS:
            raise NotImplementedError(f'anchor: dim {dim} must be 64, 128, 192 or 256')
        if len(cbs) < c.D or len(norms) < c.D:
            raise ValueError(f'anchor: {len(cbs)} codebooks / {len(norms)} norms for depth {c.D}')
        for cb, cn in zip(cbs[:c.D], norms[:c.D]):
            if tuple(cb.shape) != (c.vocab_size, dim) or tuple(cn.shape) != (c.vocab_size,):
                raise ValueError(f'anchor: codebook of shape {tuple(cb.shape)} with norms {tuple(cn.shape)}; expected ({c.vocab_size}, {dim}) '
                                 f'and ({c.vocab_size},)')
        self._on_my_device(z, *cbs[:c.D], *norms[:c.D])
        w = torch.as_tensor(weight, dtype=torch.float32, device='cpu').reshape(-1).contiguous()
        n = c.H * c.W * c.D * (B if per_image else 1)
        if w.numel() != n:
            raise ValueError(f'anchor: {w.numel()} weights; expected {n}')
        z = z.contiguous()
        # (the tensors and arrays the library reads, alive until the call returns)
        return z, _ptr_array(cbs[:c.D]), _ptr_array(norms[:c.D]), dim, w, int(per_image), cbs, norms

    def kv_bytes(self):
        """device bytes currently reserved for the KV caches of the handle (rqamd_rqt_kv_bytes)"""
        n = C.c_int64()
        check(self._L.rqamd_rqt_kv_bytes(self._h, C.byref(n)), self._L)
        return n.value

    def arm_trunc(self, min_p, typical_p, per_image=False):
        """rqamd_rqt_sample_trunc for the NEXT sample / sample_masked / sample_guided / sample_rows call of this object: min-p and
        locally typical sampling, host sequences of D floats (per_image: B * D, image-major, in front of sample_rows only), each or
        None = off.  (A method rather than an argument of the four: their argument lists stay as they are.)"""
        self._trunc = (min_p, typical_p, per_image)

    SCHEDULE_PARAMETERS = ('temperature', 'top_k', 'top_p', 'guidance_scale', 'min_p', 'typical_p')

    def arm_schedule(self, per_image=False, **tables):
        """rqamd_rqt_sample_schedule for the NEXT sample / sample_masked / sample_guided / sample_rows call of this object: sampling
        schedules over positions and depths.  Keywords of SCHEDULE_PARAMETERS, each a flat host sequence or tensor of H * W * D values in raster
        order, depth last (per_image: B * H * W * D, image-major) or None: that parameter comes from the call's own arguments.
        No keyword (or all None) disarms."""
        bad = set(tables) - set(self.SCHEDULE_PARAMETERS)
        if bad:
            raise TypeError(f'arm_schedule: unknown parameter {sorted(bad)}')
        self._sched = (dict(tables), bool(per_image)) if any(v is not None for v in tables.values()) else None

    def _sample_call(self, partial, call, want_logp, guided=False):
        """one sampling call; want_logp: armed through rqamd_rqt_sample_logp first (inside the same attempt: a failed call consumes the
        arming) -> (draw, model, model_uncond or None), (B,H,W,D) fp32 each, else None.  An arm_trunc() / arm_schedule() before the call
        is passed on to rqamd_rqt_sample_trunc / rqamd_rqt_sample_schedule the same way, and consumed"""
        trunc, self._trunc = getattr(self, '_trunc', None), None
        sched, self._sched = getattr(self, '_sched', None), None
        fan, self._shared = getattr(self, '_shared', 0), 0
        try:
            comp = self._compose_arrays(partial.shape[0])
            anc = self._anchor_arrays(partial.shape[0])
        except Exception:
            self._trunc = self._sched = self._anchor = None
            raise
        if anc is not None:
            unanchored = call

            def call(anc=anc):
                rc = self._L.rqamd_rqt_sample_anchor(self._h, ptr(anc[0], torch.float32), anc[1], anc[2], anc[3],
                                                     C.cast(anc[4].data_ptr(), C.c_void_p), anc[5])
                return rc if rc != 0 else unanchored()
        if comp is not None:
            if not guided:
                raise ValueError('extra conditions armed in front of an unguided call')
            uncomposed = call

            def call(comp=comp):                     # (comp: the arrays and tensors the library reads, alive until the call returns)
                rc = self._L.rqamd_rqt_sample_compose(self._h, comp[0], comp[1], comp[2])
                return rc if rc != 0 else uncomposed()
        if fan:
            unshared = call

            def call():
                rc = self._L.rqamd_rqt_sample_shared(self._h, fan)
                return rc if rc != 0 else unshared()
        if sched is not None:
            n = self.cfg.H * self.cfg.W * self.cfg.D * (partial.shape[0] if sched[1] else 1)
            sarrs, host = [], []                     # (host tensors: the arrays the library reads, alive until the call returns)
            for name in self.SCHEDULE_PARAMETERS:
                v = sched[0].get(name)
                if v is None:
                    sarrs.append(None)
                    continue
                t = torch.as_tensor(v, dtype=torch.int32 if name == 'top_k' else torch.float32, device='cpu').reshape(-1).contiguous()
                if t.numel() != n:
                    raise ValueError(f'arm_schedule: {name} has {t.numel()} values; expected {n}')
                host.append(t)
                sarrs.append(C.cast(t.data_ptr(), C.POINTER(C.c_int if name == 'top_k' else C.c_float)))
            unscheduled = call

            def call(host=host):
                rc = self._L.rqamd_rqt_sample_schedule(self._h, *sarrs, int(sched[1]))
                return rc if rc != 0 else unscheduled()
        if trunc is not None and (trunc[0] is not None or trunc[1] is not None):
            arrs = [None if v is None else (C.c_float * len(v))(*[float(x) for x in v]) for v in trunc[:2]]
            inner = call

            def call():
                rc = self._L.rqamd_rqt_sample_trunc(self._h, arrs[0], arrs[1], int(bool(trunc[2])))
                return rc if rc != 0 else inner()
        if not want_logp:
            self._run(call)
            return None
        draw, model = (torch.empty(partial.shape, dtype=torch.float32, device=partial.device) for _ in range(2))
        model_u = torch.empty_like(model) if guided else None

        def armed():
            rc = self._L.rqamd_rqt_sample_logp(self._h, ptr(draw), ptr(model), ptr(model_u))
            return rc if rc != 0 else call()
        self._run(armed)
        return draw, model, model_u

    def sample(self, partial, cond, codebooks, start_loc, temperature, top_k, top_p, seed, offset, use_graph, want_logp=False):
        """want_logp (here and in the three forms below): also return (draw, model, model_uncond) of rqamd_rqt_sample_logp"""
        self._check(partial, cond, codebooks)
        B = partial.shape[0]
        out = torch.empty_like(partial)
        D = self.cfg.D
        cbs, tk, tp = _ptr_array(codebooks[:D]), _int_array(top_k[:D]), (C.c_float * D)(*[float(p) for p in top_p[:D]])
        lp = self._sample_call(partial, lambda: self._L.rqamd_rqt_sample(
            self._h, ptr(partial, torch.int64), ptr(cond, torch.int64), B, cbs, int(start_loc[0]), int(start_loc[1]), float(temperature), tk, tp,
            int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(bool(use_graph)), ptr(out), stream_of(partial)), want_logp)
        return (out, lp) if want_logp else out

    def sample_masked(self, partial, keep, pos_active, cond, codebooks, temperature, top_k, top_p, seed, offset, use_graph, want_logp=False):
        """rqamd_rqt_sample_masked: `keep` (B,H,W,D) uint8 on the engine's device, nonzero = the code of `partial` is kept; `pos_active`
        a host sequence of H * W flags (0: every code of the position is kept in every row -- the caller's promise) or None."""
        self._check(partial, cond, codebooks)
        if keep is None:
            kp = None                                    # (the library refuses it: RQAMD_ERR_INVALID)
        else:
            if keep.dtype != torch.uint8 or tuple(keep.shape) != tuple(partial.shape):
                raise ValueError(f'keep of shape {tuple(keep.shape)} / {keep.dtype}; expected {tuple(partial.shape)} / torch.uint8')
            self._on_my_device(keep)
            kp = ptr(keep, torch.uint8)
        B = partial.shape[0]
        c = self.cfg
        pa = None
        if pos_active is not None:
            if len(pos_active) != c.H * c.W:
                raise ValueError(f'pos_active has {len(pos_active)} entries; expected {c.H * c.W}')
            pa = (C.c_uint8 * (c.H * c.W))(*[1 if a else 0 for a in pos_active])
        out = torch.empty_like(partial)
        D = c.D
        cbs, tk, tp = _ptr_array(codebooks[:D]), _int_array(top_k[:D]), (C.c_float * D)(*[float(p) for p in top_p[:D]])
        lp = self._sample_call(partial, lambda: self._L.rqamd_rqt_sample_masked(
            self._h, ptr(partial, torch.int64), kp, pa, ptr(cond, torch.int64), B, cbs, float(temperature), tk, tp, int(seed) & (2 ** 64 - 1),
            int(offset) & (2 ** 64 - 1), int(bool(use_graph)), ptr(out), stream_of(partial)), want_logp)
        return (out, lp) if want_logp else out

    def sample_guided(self, partial, keep, pos_active, cond, uncond, codebooks, start_loc, temperature, guidance_scale, top_k, top_p,
                      seed, offset, use_graph, want_logp=False):
        """rqamd_rqt_sample_guided: classifier-free guidance over the B images of `partial` (2B engine rows; rows B.. conditioned on
        `uncond`, None = zeros as for `cond`).  `keep` / `pos_active` as in sample_masked, or None: nothing kept."""
        self._check(partial, cond, codebooks)
        if uncond is not None:
            want = (self._cond_rows(partial.shape[0]), max(self.cfg.block_size_cond, 1))
            if tuple(uncond.shape) != want:
                raise ValueError(f'uncond of shape {tuple(uncond.shape)}; expected {want}')
            self._on_my_device(uncond)
        if not math.isfinite(float(guidance_scale)):
            raise ValueError(f'guidance_scale {guidance_scale} is not finite')
        kp = None
        if keep is not None:
            if keep.dtype != torch.uint8 or tuple(keep.shape) != tuple(partial.shape):
                raise ValueError(f'keep of shape {tuple(keep.shape)} / {keep.dtype}; expected {tuple(partial.shape)} / torch.uint8')
            self._on_my_device(keep)
            kp = ptr(keep, torch.uint8)
        B = partial.shape[0]
        c = self.cfg
        pa = None
        if pos_active is not None:
            if len(pos_active) != c.H * c.W:
                raise ValueError(f'pos_active has {len(pos_active)} entries; expected {c.H * c.W}')
            pa = (C.c_uint8 * (c.H * c.W))(*[1 if a else 0 for a in pos_active])
        out = torch.empty_like(partial)
        D = c.D
        cbs, tk, tp = _ptr_array(codebooks[:D]), _int_array(top_k[:D]), (C.c_float * D)(*[float(p) for p in top_p[:D]])
        lp = self._sample_call(partial, lambda: self._L.rqamd_rqt_sample_guided(
            self._h, ptr(partial, torch.int64), kp, pa, ptr(cond, torch.int64), ptr(uncond, torch.int64), B, cbs, int(start_loc[0]),
            int(start_loc[1]), float(temperature), float(guidance_scale), tk, tp, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
            int(bool(use_graph)), ptr(out), stream_of(partial)), want_logp, guided=True)
        return (out, lp) if want_logp else out

    def sample_rows(self, partial, keep, pos_active, cond, uncond, codebooks, start_loc, temperature, top_k, top_p, guidance_scale,
                    seeds, seed, offset, use_graph, want_logp=False):
        """rqamd_rqt_sample_rows: sampling parameters per image.  temperature (B,), top_k (B, D), top_p (B, D), guidance_scale (B,) or
        None (with uncond None: unguided) and seeds (B,) or None are HOST sequences (nested for the two (B, D) tables); `keep` /
        `pos_active` as in sample_masked or None, `uncond` as in sample_guided.  Image b is drawn as the scalar entry point draws row
        b with b's values; with seeds, from Philox key seeds[b] whatever its place in the batch (seed / offset unused)."""
        self._check(partial, cond, codebooks)
        B = partial.shape[0]
        c = self.cfg
        D = c.D
        if uncond is not None:
            want = (self._cond_rows(B), max(c.block_size_cond, 1))
            if tuple(uncond.shape) != want:
                raise ValueError(f'uncond of shape {tuple(uncond.shape)}; expected {want}')
            self._on_my_device(uncond)
            if guidance_scale is None:
                raise ValueError('sample_rows: uncond needs guidance_scale')
        T = [float(t) for t in temperature]
        tk = [int(k) for row in top_k for k in row]
        tp = [float(p) for row in top_p for p in row]
        gs = None if guidance_scale is None else [float(s) for s in guidance_scale]
        sd = None if seeds is None else [int(s) for s in seeds]
        if len(T) != B or len(tk) != B * D or len(tp) != B * D or (gs is not None and len(gs) != B) or (sd is not None and len(sd) != B):
            raise ValueError(f'sample_rows: per-image values of the wrong shape for {B} images of depth {D}')
        if not all(math.isfinite(t) and t > 0 for t in T):
            raise ValueError('sample_rows: every temperature must be > 0 and finite')
        if gs is not None and not all(math.isfinite(s) for s in gs):
            raise ValueError('sample_rows: every guidance_scale must be finite')
        if sd is not None and any(s < 0 or s >= 2 ** 64 for s in sd):
            raise ValueError('sample_rows: seeds must be in 0 .. 2**64 - 1')
        kp = None
        if keep is not None:
            if keep.dtype != torch.uint8 or tuple(keep.shape) != tuple(partial.shape):
                raise ValueError(f'keep of shape {tuple(keep.shape)} / {keep.dtype}; expected {tuple(partial.shape)} / torch.uint8')
            self._on_my_device(keep)
            kp = ptr(keep, torch.uint8)
        pa = None
        if pos_active is not None:
            if len(pos_active) != c.H * c.W:
                raise ValueError(f'pos_active has {len(pos_active)} entries; expected {c.H * c.W}')
            pa = (C.c_uint8 * (c.H * c.W))(*[1 if a else 0 for a in pos_active])
        out = torch.empty_like(partial)
        cbs = _ptr_array(codebooks[:D])
        aT, ak, ap = (C.c_float * B)(*T), (C.c_int * (B * D))(*tk), (C.c_float * (B * D))(*tp)
        ag = None if gs is None else (C.c_float * B)(*gs)
        asd = None if sd is None else (C.c_uint64 * B)(*sd)
        lp = self._sample_call(partial, lambda: self._L.rqamd_rqt_sample_rows(
            self._h, ptr(partial, torch.int64), kp, pa, ptr(cond, torch.int64), ptr(uncond, torch.int64), B, cbs, int(start_loc[0]),
            int(start_loc[1]), aT, ak, ap, ag, asd, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(bool(use_graph)), ptr(out),
            stream_of(partial)), want_logp, guided=gs is not None)
        return (out, lp) if want_logp else out

    def graph_captures(self):
        """position graphs this handle has captured so far (rqamd_rqt_graph_captures); a call that only replays leaves it unchanged"""
        n = C.c_int64()
        check(self._L.rqamd_rqt_graph_captures(self._h, C.byref(n)), self._L)
        return n.value

    def logits(self, codes, cond, codebooks):
        self._check(codes, cond, codebooks)
        B = codes.shape[0]
        c = self.cfg
        out = torch.empty((B, c.H, c.W, c.D, c.vocab_size), dtype=torch.float32, device=codes.device)
        cbs = _ptr_array(codebooks[:c.D])
        self._run(lambda: self._L.rqamd_rqt_logits(self._h, ptr(codes, torch.int64), ptr(cond, torch.int64), B, cbs,
                                                 ptr(out), stream_of(codes)))
        return out

    def forward(self, codes, cond, codebooks):
        """(seq_logits (B,H,W,D,V), cond_logits (B, block_size_cond-1, vocab_size_cond)) -- text-conditioned models"""
        self._check(codes, cond, codebooks)
        B = codes.shape[0]
        c = self.cfg
        out = torch.empty((B, c.H, c.W, c.D, c.vocab_size), dtype=torch.float32, device=codes.device)
        cl = torch.empty((B, c.block_size_cond - 1, max(c.vocab_size_cond, 1)), dtype=torch.float32, device=codes.device)
        cbs = _ptr_array(codebooks[:c.D])
        self._run(lambda: self._L.rqamd_rqt_forward(self._h, ptr(codes, torch.int64), ptr(cond, torch.int64), B, cbs,
                                                  ptr(out), ptr(cl), stream_of(codes)))
        return out, cl

    # ---- one pass over all positions (rqamd_rqt_forward_onepass / rqamd_rqt_log_probs): no KV cache, a workspace of its own
    def forward_onepass(self, codes, cond, codebooks):
        """seq_logits (B,H,W,D,V), or (seq_logits, cond_logits (B, block_size_cond-1, vocab_size_cond)) for text-conditioned models"""
        self._check(codes, cond, codebooks)
        B = codes.shape[0]
        c = self.cfg
        out = torch.empty((B, c.H, c.W, c.D, c.vocab_size), dtype=torch.float32, device=codes.device)
        cl = None
        if c.block_size_cond > 1:
            cl = torch.empty((B, c.block_size_cond - 1, max(c.vocab_size_cond, 1)), dtype=torch.float32, device=codes.device)
        cbs = _ptr_array(codebooks[:c.D])
        self._run(lambda: self._L.rqamd_rqt_forward_onepass(self._h, ptr(codes, torch.int64), ptr(cond, torch.int64), B, cbs,
                                                          ptr(out), ptr(cl), stream_of(codes)))
        return out if cl is None else (out, cl)

    def log_probs(self, codes, cond, codebooks):
        """log p(code) of every code (B,H,W,D) fp32, or (that, log p(cond[t+1] | cond[:t+1]) (B, block_size_cond-1)) for
        text-conditioned models; the (B,H,W,D,V) logits are never materialised"""
        self._check(codes, cond, codebooks)
        B = codes.shape[0]
        c = self.cfg
        out = torch.empty((B, c.H, c.W, c.D), dtype=torch.float32, device=codes.device)
        cl = None
        if c.block_size_cond > 1:
            if cond is None:
                raise ValueError('log_probs of a text-conditioned model needs cond')
            cl = torch.empty((B, c.block_size_cond - 1), dtype=torch.float32, device=codes.device)
        cbs = _ptr_array(codebooks[:c.D])
        self._run(lambda: self._L.rqamd_rqt_log_probs(self._h, ptr(codes, torch.int64), ptr(cond, torch.int64), B, cbs,
                                                    ptr(out), ptr(cl), stream_of(codes)))
        return out if cl is None else (out, cl)

    def soft_loss(self, codes, cond, codebooks, soft_targets=None, z=None, norms=None, temp=1.0):
        """rqamd_rqt_soft_loss: the soft-target cross entropy of every code (B,H,W,D) fp32 against `soft_targets` (B,H,W,D,V) fp32, or
        against the soft codes of the features `z` (B,H,W,input_embed_dim) fp32 at temperature `temp` (norms: rq_code_norms of every
        codebook), formed inside the engine; (that, cond_logp) for text-conditioned models, as log_probs.  Neither the logits nor (from z)
        the targets are materialised."""
        self._check(codes, cond, codebooks)
        B = codes.shape[0]
        c = self.cfg
        if (soft_targets is None) == (z is None):
            raise ValueError('soft_loss: exactly one of soft_targets and z must be given')
        nrm = None
        if soft_targets is not None:
            if tuple(soft_targets.shape) != (B, c.H, c.W, c.D, c.vocab_size):
                raise ValueError(f'soft_targets of shape {tuple(soft_targets.shape)}; expected {(B, c.H, c.W, c.D, c.vocab_size)}')
            self._on_my_device(soft_targets)
        else:
            if tuple(z.shape) != (B, c.H, c.W, c.input_embed_dim):
                raise ValueError(f'z of shape {tuple(z.shape)}; expected {(B, c.H, c.W, c.input_embed_dim)}')
            if norms is None or len(norms) < c.D:
                raise ValueError(f'soft_loss: z needs the code norms of the {c.D} codebooks')
            for d in range(c.D):
                if tuple(codebooks[d].shape) != (c.vocab_size, c.input_embed_dim) or tuple(norms[d].shape) != (c.vocab_size,):
                    raise NotImplementedError(f'soft_loss: codebook {d} of shape {tuple(codebooks[d].shape)}; the targets need codebooks of '
                                              f'exactly vocab_size = {c.vocab_size} codes of dim {c.input_embed_dim} with their norms')
            if not (float(temp) > 0):
                raise ValueError(f'soft_loss: temp = {temp} must be > 0')
            self._on_my_device(z, *norms[:c.D])
            nrm = _ptr_array(norms[:c.D])
        out = torch.empty((B, c.H, c.W, c.D), dtype=torch.float32, device=codes.device)
        cl = None
        if c.block_size_cond > 1:
            if cond is None:
                raise ValueError('soft_loss of a text-conditioned model needs cond')
            cl = torch.empty((B, c.block_size_cond - 1), dtype=torch.float32, device=codes.device)
        cbs = _ptr_array(codebooks[:c.D])
        self._run(lambda: self._L.rqamd_rqt_soft_loss(self._h, ptr(codes, torch.int64), ptr(cond, torch.int64), B, cbs,
                                                    ptr(soft_targets, torch.float32), ptr(z, torch.float32), nrm, float(temp), ptr(out), ptr(cl),
                                                    stream_of(codes)))
        return out if cl is None else (out, cl)

    def set_option(self, name, value):
        """options the config struct does not carry (include/rqamd.h: rqamd_rqt_set_option), e.g. 'fwd.chunk_rows'"""
        check(self._L.rqamd_rqt_set_option(self._h, name.encode(), int(value)), self._L)

    # ---- stepping form: the caller draws the samples (rqamd_rqt_step_*)
    def step_begin(self, partial, cond, codebooks):
        self._check(partial, cond, codebooks)
        self._step = (partial.shape[0], partial.device, [cb for cb in codebooks[:self.cfg.D]])     # keeps the codebooks alive
        cbs = _ptr_array(self._step[2])
        self._run(lambda: self._L.rqamd_rqt_step_begin(self._h, ptr(partial, torch.int64), ptr(cond, torch.int64), partial.shape[0], cbs,
                                                     stream_of(partial)))

    def step_prefill(self, n_pos):
        """directly after step_begin: the KV cache of positions 0 .. n_pos-1 from the given codes in one pass (rqamd_rqt_step_prefill) --
        stands for step_logits(p, -1), p < n_pos; the next step is (n_pos, 0)"""
        step = getattr(self, '_step', None)
        dev = step[1] if step else self.device
        with on_device_of(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream if dev.type == 'cuda' else 0)
            check(self._L.rqamd_rqt_step_prefill(self._h, int(n_pos), st), self._L)

    def step_run(self, p0, p1):
        """at position p0 >= 1 with no head step of p0 taken: the KV cache of positions p0 .. p1-1 from the codes in one pass
        (rqamd_rqt_step_run) -- stands for step_logits(p, -1), p0 <= p < p1; the next step is (p1, 0)"""
        step = getattr(self, '_step', None)
        dev = step[1] if step else self.device
        with on_device_of(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream if dev.type == 'cuda' else 0)
            check(self._L.rqamd_rqt_step_run(self._h, int(p0), int(p1), st), self._L)

    def attn_extend(self, qkv, kc, vc, y, n_img, R, T0, nh, Tcap):
        """the cache-extending attention alone in this engine's build (bf16, or fp16 behind half=True): dbg_rqt_attn_extend"""
        return dbg_rqt_attn_extend(qkv, kc, vc, y, n_img, R, T0, nh, Tcap, half=self.half)

    def step_logits(self, pos, d):
        """logits (B, V) fp32 of step (pos, d) -- a view of the engine's workspace, valid until the next engine call; d < 0:
        body stack only (returns None)."""
        B, dev, _ = self._step
        out = C.c_void_p()
        with on_device_of(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream if dev.type == 'cuda' else 0)
            check(self._L.rqamd_rqt_step_logits(self._h, int(pos), int(d), C.byref(out), st), self._L)
        if d < 0:
            return None
        return _view_f32(out.value, (B, self.cfg.vocab_size), dev)

    def step_set_code(self, pos, d, codes):
        B, dev, _ = self._step
        if tuple(codes.shape) != (B,):
            raise ValueError(f'codes of shape {tuple(codes.shape)}; expected ({B},)')
        with on_device_of(dev):
            check(self._L.rqamd_rqt_step_set_code(self._h, int(pos), int(d), ptr(codes.contiguous(), torch.int64), stream_of(codes)), self._L)

    def step_end(self):
        B, dev, _ = self._step
        c = self.cfg
        out = torch.empty((B, c.H, c.W, c.D), dtype=torch.int64, device=dev)
        with on_device_of(dev):
            check(self._L.rqamd_rqt_step_end(self._h, ptr(out), stream_of(out)), self._L)
        self._step = None
        return out

    def set_profile(self, mode):
        """0 / False: off; 1 / True: HIP events around every GEMM / attention launch (eager launches); 2: skip the GEMM launches (graphs
        stay on) -- a sampling pass timed with and without them gives the GEMMs' time inside the graphs."""
        check(self._L.rqamd_rqt_set_profile(self._h, int(mode)), self._L)

    def get_profile(self):
        ms, n, by, fl = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        check(self._L.rqamd_rqt_get_profile(self._h, C.byref(ms), C.byref(n), C.byref(by), C.byref(fl)), self._L)
        ams, an = C.c_double(), C.c_int64()
        check(self._L.rqamd_rqt_get_profile_attn(self._h, C.byref(ams), C.byref(an)), self._L)
        return dict(gemm_ms_total=ms.value, gemm_launches=n.value, gemm_bytes=by.value, gemm_flops=fl.value,
                    attn_ms_total=ams.value, attn_launches=an.value)
