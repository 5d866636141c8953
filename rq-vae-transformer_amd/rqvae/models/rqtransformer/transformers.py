"""Stage-2 model: API mirror of rqvae/models/rqtransformer/transformers.py:34-369 of the reference.

``sample`` keeps the reference signature (transformers.py:294-308) and semantics -- partial_sample is
cloned not mutated, rows before start_loc are kept, per-depth top-k/top-p lists, cond None -> zeros --
but the 256-step loop runs inside librqamd's sampling engine (csrc/engine_rqt.hip): one C call enqueues
the whole loop on a side stream, replaying one captured hipGraph per spatial position, with the
sampler on the device (no host sync per step).  Weights, GEMM operands and the KV cache are bf16 by default
(BASELINE.json's compute dtype) and IEEE fp16 under ``amp=True`` -- the reference's ``amp`` is fp16 autocast
(transformers.py:21,206; main_sampling_fid.py:216 passes it) and the engine's fp16 build (librqamd_f16.so) is what
serves it: three more mantissa bits than bf16, the same MFMA rate; accumulation / residual stream / LayerNorm /
softmax / logits are fp32 either way.  Arguments of ``sample`` that cannot mean here what they mean upstream
are never ignored silently: ``cached=False`` runs a real uncached loop (every step recomputes all logits; the reference's own
cross-check of its cache, transformers.py:352-356); ``is_tqdm`` / ``desc`` have nothing to report on (the
whole loop is one asynchronous C call) and ``fast`` is unused by the reference itself."""
import contextlib
import functools
import inspect
import math
import os
from collections import OrderedDict, namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _native
from .._sync import SideStream, push_all, signature
from ..interfaces import Stage2Model
from .attentions import AttentionStack
from .configs import resolve
from .primitives import BatchLinear, LogitMask, TupleEmbedding


class _AttrView(dict):
    """resolved config with attribute access (the reference keeps an OmegaConf node in self.config)"""
    __getattr__ = dict.__getitem__

    def copy(self):
        return _attr(dict(self))


def _attr(d):
    return _AttrView({k: _attr(v) if isinstance(v, dict) else v for k, v in d.items()})


# sample(return_log_probs=True) / sample_guided(...): (B,H,W,D) fp32 each.  draw: log-probability of every drawn code in the distribution
# it was drawn from (after guidance, temperature, top-k, top-p, renormalisation), +0.0 for kept codes; model: log_softmax of the raw
# conditional logits at the code, NaN where the head did not run; model_uncond: the same under `uncond` (None when unguided)
SampleLogProbs = namedtuple('SampleLogProbs', ['draw', 'model', 'model_uncond'])


def _truncation_keywords(fn):
    """sample() / sample_guided() also take ``min_p=`` / ``typical_p=`` as keywords: the call then runs inside ``self.truncation(...)``.
    (A wrapper, so that the argument lists of the two methods stay the reference's plus keep_mask / uncond / guidance_scale, as for
    seeds() and return_log_probs(); inspect.signature shows the method underneath.)"""
    @functools.wraps(fn)
    def with_truncation(self, *args, min_p=None, typical_p=None, **kwargs):
        if min_p is None and typical_p is None:
            return fn(self, *args, **kwargs)
        with self.truncation(min_p=min_p, typical_p=typical_p):
            return fn(self, *args, **kwargs)
    return with_truncation


def _shared_prompt(fn):
    """sample() / sample_guided() inside ``with self.shared_cond(n)``: the checks of the shared-prompt form, made before anything runs, and
    the mark that makes _cond() / _sampling_eng() treat `cond` / `uncond` as one row per group for the duration of this call only."""
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def shared(self, *args, **kwargs):
        n = self._shared_cond
        if not n or self._shared_live:
            return fn(self, *args, **kwargs)
        a = sig.bind(self, *args, **kwargs)
        a.apply_defaults()
        a = a.arguments
        if self.sampler == 'torch' or not a['cached']:
            raise NotImplementedError("shared_cond() needs the engine's own sampling loop: sampler='torch' and cached=False have no shared-prompt form")
        B = a['partial_sample'].shape[0]
        if B % n:
            raise ValueError(f'shared_cond({n}): partial_sample has {B} images, not a multiple of {n}')
        for name in ('cond', 'uncond'):
            c = a.get(name)
            if c is not None and (c.shape[0] != B // n or c.numel() != (B // n) * self.block_size_cond):
                raise ValueError(f'shared_cond({n}): {name} of shape {tuple(c.shape)}; expected {(B // n, self.block_size_cond)} (one row per group of {n} images)')
        self._shared_live = n
        try:
            return fn(self, *args, **kwargs)
        finally:
            self._shared_live = 0
            for eng, _ in self._engines.values():
                eng.arm_shared(0)                     # (a call refused before it reached the library leaves nothing armed)
    return shared


def _anchored(fn):
    """sample() / sample_guided() inside ``with self.anchor(z, weight)``: the checks of anchored sampling, made before anything runs, and
    the mark that makes _sampling_eng() arm the engine (rqamd_rqt_sample_anchor) and the host loops fold the anchor into their logits for
    the duration of this call only."""
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def anchored(self, *args, **kwargs):
        if self._anchor is None or self._anchor_live is not None:
            return fn(self, *args, **kwargs)
        a = sig.bind(self, *args, **kwargs)
        a.apply_defaults()
        a = a.arguments
        self._anchor_live = self._anchor_args(a['partial_sample'], a['model_aux'])
        try:
            return fn(self, *args, **kwargs)
        finally:
            self._anchor_live = None
            for eng, _ in self._engines.values():
                eng.arm_anchor(None)                  # (a call refused before it reached the library leaves nothing armed)
    return anchored


def _negative_prompt(fn):
    """sample_guided() also takes ``negative=`` / ``negative_scale=`` as keywords: the call then runs inside
    ``self.extra_conds(conds=[negative], weights=[-negative_scale])`` (see extra_conds()); both the keyword and the context: ValueError.
    The checks of composed guidance that need no tensor are made here, before anything runs.  (A wrapper, as _truncation_keywords is.)"""
    @functools.wraps(fn)
    def with_negative(self, *args, negative=None, negative_scale=1.0, **kwargs):
        if negative is not None:
            if self._extra_conds is not None:
                raise ValueError('negative= given inside extra_conds(): pass the negative prompt as one of the extra conditions')
            w = negative_scale if torch.is_tensor(negative_scale) else float(negative_scale)
            with self.extra_conds(conds=[negative], weights=[-w]):
                return with_negative(self, *args, **kwargs)
        if self._extra_conds is not None:
            if self.sampler == 'torch':
                raise NotImplementedError("extra_conds() runs in the on-device sampler; sampler='torch' has no composed form")
            if self._shared_cond:
                raise NotImplementedError('extra_conds() inside shared_cond(): the extra row blocks would need group caches of their own')
        return fn(self, *args, **kwargs)
    return with_negative


class RQTransformer(Stage2Model):

    def __init__(self, config):
        super().__init__()
        cfg = resolve(config)
        if len(cfg['block_size']) != 3:
            raise ValueError("incompatible block size")
        self.block_size = torch.Size(cfg['block_size'])
        if isinstance(cfg['vocab_size'], int):
            cfg['vocab_size'] = [cfg['vocab_size']] * cfg['block_size'][2]
        if cfg['shared_tok_emb'] or cfg['shared_cls_emb']:
            assert [cfg['vocab_size'][0]] * len(cfg['vocab_size']) == list(cfg['vocab_size'])
        self.config = _attr(cfg)
        self.vocab_size = list(cfg['vocab_size'])
        # every released config sets input_emb_vqvae / head_emb_vqvae / shared_cls_emb / cumsum_depth_ctx
        # (configs/**/stage2/*.yaml:13-18); the other combinations (primitives.py) are supported by the engine as well
        E = cfg['embed_dim']
        self.vocab_size_cond = max(cfg['vocab_size_cond'], 1)
        self.block_size_cond = max(cfg['block_size_cond'], 1)
        assert not (self.block_size_cond > 1 and self.vocab_size_cond == 1)
        self.cond_emb = nn.Embedding(self.vocab_size_cond, E)
        self.tok_emb, self.input_mlp, self.head_mlp = None, None, None          # transformers.py:60-70
        if cfg['input_emb_vqvae']:
            self.input_mlp = nn.Linear(cfg['input_embed_dim'], E)
        if cfg['head_emb_vqvae']:
            self.head_mlp = nn.Linear(cfg['input_embed_dim'], E)
        if not (cfg['input_emb_vqvae'] and cfg['head_emb_vqvae']):
            if cfg['shared_tok_emb']:
                self.tok_emb = nn.Embedding(cfg['vocab_size'][0], E)
            else:
                self.tok_emb = TupleEmbedding(cfg['vocab_size'], E)
        self.pos_emb_cond = nn.Parameter(torch.zeros(1, self.block_size_cond, E))
        self.pos_emb_hw = nn.Parameter(torch.zeros(1, self.block_size[0] * self.block_size[1], E))
        self.pos_emb_d = nn.Parameter(torch.zeros(1, self.block_size[2], E))
        self.pos_emb_cond.data.normal_(mean=0.0, std=0.02)
        self.pos_emb_hw.data.normal_(mean=0.0, std=0.02)
        self.pos_emb_d.data.normal_(mean=0.0, std=0.02)
        self.embed_drop = nn.Dropout(cfg['embd_pdrop'], inplace=True)
        self.body_transformer = AttentionStack(cfg['body'])
        self.head_transformer = AttentionStack(cfg['head'])
        self.classifier = nn.Sequential(OrderedDict([
            ('layer_norm', nn.LayerNorm(E)),
            ('linear', nn.Linear(E, cfg['vocab_size'][0]) if cfg['shared_cls_emb']
             else BatchLinear(cfg['block_size'][2], E, max(cfg['vocab_size']))),
            ('logit_mask', LogitMask(cfg['vocab_size'], value=-1e6)),
        ]))
        if cfg['block_size_cond'] > 1:
            self.cond_classifier = nn.Sequential(OrderedDict([
                ('layer_norm', nn.LayerNorm(E)),
                ('linear', nn.Linear(E, cfg['vocab_size_cond'])),
            ]))
        self._cache = None
        self._engines = {}                               # amp (False: bf16 engine, True: fp16 engine) -> (engine, parameter signature)
        self._side = SideStream()
        self.use_graph = os.environ.get('RQAMD_GRAPH', '1') != '0'
        # 'philox' (default): on-device sampler inside the captured graphs; 'torch': host loop + torch.multinomial (see sample)
        self.sampler = os.environ.get('RQAMD_SAMPLER', 'philox')
        # how forward() / teacher_forced_logits() run: 'stepped' (default): the cached sampler driven over the given codes, B rows per
        # launch; 'one_pass' (or RQAMD_FORWARD=one_pass): every position at once, no KV cache (rqamd_rqt_forward_onepass) -- same
        # arithmetic, other GEMM tiles.  cached_forward and sample (cached or not) always step.
        self.forward_mode = os.environ.get('RQAMD_FORWARD', 'stepped')
        # how sample() / sample_guided() / a restarted cached_forward bring the GIVEN leading positions (before start_loc, or a fully
        # kept leading run of keep_mask) into the body stack's KV cache: 'stepped' (default): one body-only step per position;
        # 'one_pass' (or RQAMD_PREFIX=one_pass): conditioning tokens and prefix codes through the body stack at once, the way the
        # reference's first cached step does (engine option "prefix.one_pass" / rqamd_rqt_step_prefill).  Same arithmetic through other
        # GEMM tiles: the codes drawn after the prefix differ from the stepped mode's wherever a draw was close; filters and Philox
        # counters are the same.  sample(cached=False) has no cache and is untouched.
        self.prefix_mode = os.environ.get('RQAMD_PREFIX', 'stepped')
        # how the same calls bring kept runs that are NOT leading (keep_mask: the left columns of every row, the rows between two drawn
        # bands, the rim of a hole -- positions whose codes are kept in every image) into the cache: 'stepped' (default): one body-only
        # step per position; 'one_pass' (or RQAMD_KEPT_RUNS=one_pass): every such run of two positions or more through the body stack
        # at once (engine option "masked.run_prefill" / rqamd_rqt_step_run).  Independent of prefix_mode; numerics as there.  8-bit
        # caches (RQAMD_KV), body head sizes other than 64 and shared_cond() calls stay stepped.
        self.kept_run_mode = os.environ.get('RQAMD_KEPT_RUNS', 'stepped')
        self._return_log_probs = False                   # inside `with self.return_log_probs()`: sample() also returns SampleLogProbs
        self._image_seeds = None                         # per-image Philox seeds of the sample() calls inside `with self.seeds(...)`
        self._truncation = (None, None)                  # (min_p, typical_p) of the sample() calls inside `with self.truncation(...)`
        self._schedule = None                            # {parameter: tensor} of the sample() calls inside `with self.schedule(...)`
        self._shared_cond = 0                            # images per prompt of the sample() calls inside `with self.shared_cond(n)`
        self._shared_live = 0                            # ... while such a call runs (_shared_prompt)
        self._extra_conds = None                         # (conds, weights) of the sample_guided() calls inside `with self.extra_conds(...)`
        self._anchor = None                              # (z, weight) of the sample() calls inside `with self.anchor(...)`
        self._anchor_live = None                         # ... checked and broadcast, while such a call runs (_anchored)

    # ------------------------------------------------------------------ engine plumbing
    @property
    def _engine(self):
        """the default (bf16) engine, or None before its first use (bench.py / scripts read its profile counters)"""
        return self._engines.get(False, (None, None))[0]

    @_engine.setter
    def _engine(self, value):
        if value is None:
            self._engines.pop(False, None)
        else:
            self._engines[False] = (value, None)

    def _eng(self, amp=False):
        """The native engine for this precision: amp=False -> bf16 (librqamd.so), amp=True -> IEEE fp16 (librqamd_f16.so).  Each keeps its
        own packed copy of the parameters (pushed again whenever the module's tensors change) and its own KV cache / graphs."""
        amp = bool(amp)
        sig = signature(self)
        eng, esig = self._engines.get(amp, (None, None))
        if eng is not None and eng.device != self.pos_emb_hw.device:
            eng.close()                                 # the module moved (model.to(other device)): rebuild there
            eng = None
        if eng is None or sig != esig:
            self._cf = None                             # (a cached_forward sequence does not survive an engine rebuild / parameter push)
            if eng is None:
                c = self.config
                gb, gh = c.body.block.gelu == 'v2', c.head.block.gelu == 'v2'
                gelu_code = 1 if (gb and gh) else 3 if gb else 2 if gh else 0      # (the stacks may differ: include/rqamd.h)
                eng = _native.RqtEngine(
                    embed_dim=c.embed_dim, n_head=c.body.block.n_head, n_layer_body=c.body.n_layer, n_layer_head=c.head.n_layer,
                    vocab_size=max(self.vocab_size), input_embed_dim=c.input_embed_dim, vocab_size_cond=self.vocab_size_cond,
                    block_size_cond=self.block_size_cond, block_size=list(self.block_size), gelu_v2=gelu_code,
                    device=self.pos_emb_hw.device, input_emb_vqvae=c.input_emb_vqvae, head_emb_vqvae=c.head_emb_vqvae,
                    shared_tok_emb=c.shared_tok_emb, shared_cls_emb=c.shared_cls_emb, cumsum_depth_ctx=c.cumsum_depth_ctx,
                    vocab_sizes=self.vocab_size, half=amp, n_head_head=c.head.block.n_head)
            push_all(self, eng)
            # bias-free layers (attn_bias / mlp_bias = False): the engine's epilogues always add a bias vector -- zeros here
            dev = self.pos_emb_hw.device
            for prefix, stack in (('body_transformer', self.body_transformer), ('head_transformer', self.head_transformer)):
                for i, blk in enumerate(stack.blocks):
                    for leaf, lin in (('attn.query', blk.attn.query), ('attn.key', blk.attn.key), ('attn.value', blk.attn.value),
                                      ('attn.proj', blk.attn.proj), ('mlp.0', blk.mlp[0]), ('mlp.2', blk.mlp[2])):
                        if lin.bias is None:
                            eng.set_param(f'{prefix}.blocks.{i}.{leaf}.bias', torch.zeros(lin.out_features, device=dev))
            self._engines[amp] = (eng, sig)
        return eng

    def _prefix_one_pass(self):
        if self.prefix_mode not in ('stepped', 'one_pass'):
            raise ValueError(f"prefix_mode = {self.prefix_mode!r} ('stepped' or 'one_pass')")
        return self.prefix_mode == 'one_pass'

    def _kept_runs_one_pass(self):
        if self.kept_run_mode not in ('stepped', 'one_pass'):
            raise ValueError(f"kept_run_mode = {self.kept_run_mode!r} ('stepped' or 'one_pass')")
        return self.kept_run_mode == 'one_pass'

    def _sampling_eng(self, amp=False):
        """_eng(amp) with the engine's "prefix.one_pass" / "masked.run_prefill" options following self.prefix_mode / self.kept_run_mode
        (touched only when they have to change: a handle of a model that never leaves the default never sees the options), and -- inside shared_cond(n) only -- armed for a
        shared-prompt call (the call consumes the arming, and _shared_prompt disarms whatever a refused call left: outside the context
        the engine is not touched)"""
        want, want_runs = self._prefix_one_pass(), self._kept_runs_one_pass()
        eng = self._eng(amp)
        if getattr(eng, '_prefix_one_pass', False) != want:
            eng.set_option('prefix.one_pass', int(want))
            eng._prefix_one_pass = want
        if getattr(eng, '_kept_runs_one_pass', False) != want_runs:
            eng.set_option('masked.run_prefill', int(want_runs))
            eng._kept_runs_one_pass = want_runs
        if self._shared_live:
            eng.arm_shared(self._shared_live)           # the next sampling call of the engine is a shared-prompt call
        if self._anchor_live is not None:               # ... an anchored call (the host loops never reach it: _anchored disarms)
            a = self._anchor_live
            eng.arm_anchor(a['z'], a['cbs'], a['norms'], a['w'].reshape(-1), a['per_image'])
        return eng

    def _cond_rows(self, B):
        """rows of cond / uncond for B images: B, or -- a call inside shared_cond(n) -- one per group"""
        return B // self._shared_live if self._shared_live else B

    @staticmethod
    def _codebooks(model_aux):
        """model_aux.get_code_emb_with_depth is the only thing the reference uses model_aux for
        (transformers.py:109-111); the engine gathers from the same tables directly."""
        if model_aux is None or not hasattr(model_aux, 'quantizer'):
            raise ValueError('model_aux must be the RQVAE whose codebook embeds the codes (input_emb_vqvae=True)')
        return model_aux.quantizer.codebook_list()

    def _checked_codebooks(self, model_aux):
        """the engine gathers rows `code` < vocab_size of width input_embed_dim from these tables: anything else would read
        out of bounds, so the shapes are checked here (the reference would fail in F.embedding / input_mlp)"""
        D = self.block_size[2]
        if not (self.config.input_emb_vqvae or self.config.head_emb_vqvae):
            return [self.tok_emb.weight.detach()] * D      # learned embeddings only: model_aux is not consulted (placeholders)
        cbs = self._codebooks(model_aux)
        if len(cbs) < D:
            raise ValueError(f'model_aux has {len(cbs)} codebooks, the transformer needs {D}')
        for d in range(D):
            cb = cbs[d]
            if cb.dim() != 2 or cb.shape[1] != self.config.input_embed_dim or cb.shape[0] < self.vocab_size[d]:
                raise ValueError(f'codebook {d} has shape {tuple(cb.shape)}; expected (>= {self.vocab_size[d]}, '
                                 f'{self.config.input_embed_dim})')
        return cbs[:D]

    def _cond(self, cond, B, device):
        if cond is None:
            return None                                  # engine zero-fills (transformers.py:208-209)
        return cond.reshape(self._cond_rows(B), self.block_size_cond).to(device=device, dtype=torch.long).contiguous()

    def _on_side_stream(self, device, fn):
        return self._side.run(device, fn)

    # ------------------------------------------------------------------ reference API
    def init_cache(self):
        """transformers.py:289-292 -- caches are engine-side and reset by every sample()/forward(); a cached_forward sequence in
        progress ends here."""
        self._cache = {'spatial_ctx_hw': None}
        self._cf = None

    @torch.no_grad()
    def cached_forward(self, xs, model_aux=None, cond=None, amp=False, sample_loc=(0, 0, 0)):
        """transformers.py:190-287: logits (B, vocab_size) fp32 of ONE step (h, w, d) from the KV caches of the steps before it, over
        the engine's stepping entry points (rqamd_rqt_step_begin / _step_logits / _step_set_code: the arithmetic of sample()).  As in
        the reference the calls of a sequence come in sampling order after init_cache(): a call with d == 0 that does not continue
        the previous call starts a sequence -- the codes of the positions before (h, w) are taken from `xs` and only feed the body
        stack's KV cache (the start_loc > (0, 0) prefill, :235-239; that restart costs `pos` body-only steps, or with
        prefix_mode = 'one_pass' one pass over the prefix as in the reference, and so does any call that
        finds the engine rebuilt, the parameters pushed again or `amp` changed since the previous one) -- and a call with d > 0 must
        follow (h, w, d - 1).  `model_aux` and `cond` are read when a sequence starts; only the code of the step before is re-read
        from `xs` at a continuing call (the reference re-embeds all of `xs` every time).  `xs` holds
        the codes drawn so far, (B, h + 1 .. H, W, D) as sample() passes them (:349); the codes of the step before are read from it
        at every call, so a caller may write them in place like sample() does (:364).  The returned tensor is the caller's own."""
        (h, w, d) = (int(v) for v in sample_loc)
        (B, Hx, W, D) = xs.shape
        (H, W_, D_) = self.block_size
        assert (W, D) == (W_, D_) and h < Hx <= H and 0 <= w < W and 0 <= d < D
        pos = h * W + w
        eng = self._eng(amp)
        st = getattr(self, '_cf', None)
        if st is not None and st.get('eng') is not eng:
            st = None                                   # another engine (precision) or a rebuilt one: the sequence restarts
        if st is None or st['next'] != (pos, d) or st['B'] != B:
            if d != 0:
                raise RuntimeError(f'cached_forward(sample_loc={tuple(sample_loc)}): depth {d} must follow depth {d - 1} of the same position '
                                   '(the head stack attends its cached depths; call init_cache() and step in sampling order)')
            cbs = self._checked_codebooks(model_aux)
            full = torch.zeros((B, H, W, D), dtype=torch.long, device=xs.device)
            full[:, :Hx] = xs
            c = self._cond(cond, B, xs.device)
            if c is None:
                c = torch.zeros((B, self.block_size_cond), dtype=torch.long, device=xs.device)
            one_pass = self._prefix_one_pass()
            eng.step_begin(full.contiguous(), c, cbs)
            if one_pass and pos >= 1:
                eng.step_prefill(pos)                  # given codes: body KV cache only, in one pass (prefix_mode)
            else:
                for p in range(pos):
                    eng.step_logits(p, -1)             # given codes: body KV cache only
        elif d > 0:
            eng.step_set_code(pos, d - 1, xs[:, h, w, d - 1].to(torch.long).contiguous())
        elif pos > 0:
            hp, wp = divmod(pos - 1, W)
            eng.step_set_code(pos - 1, D - 1, xs[:, hp, wp, D - 1].to(torch.long).contiguous())
        logits = eng.step_logits(pos, d).clone()
        self._cf = {'next': (pos, d + 1) if d + 1 < D else (pos + 1, 0), 'B': B, 'eng': eng}
        return logits

    def embed_with_model_aux(self, xs, model_aux):
        xs_emb, _ = model_aux.get_code_emb_with_depth(xs)
        return xs_emb

    @torch.no_grad()
    def forward(self, xs, model_aux=None, cond=None, amp=False):
        """transformers.py:113-188: teacher-forced logits (B,H,W,D,V) fp32, computed by stepping the
        engine's cached path over the given codes (identical to the uncached pass up to rounding --
        the reference's own cached==uncached invariant, transformers.py:352-356)."""
        self._cf = None                                  # (any other engine call ends a cached_forward sequence)
        one_pass = self._one_pass()
        if self.block_size_cond > 1:
            # (seq_logits, cond_logits): cond_classifier over the body outputs of the first cond_len-1 positions
            # (transformers.py:150-153,185-186); the engine takes them from the multi-token prefill of the prefix
            (B, H, W, D) = xs.shape
            assert torch.Size([H, W, D]) == self.block_size
            eng = self._eng(amp)
            cbs = self._checked_codebooks(model_aux)
            codes = xs.to(torch.long).contiguous()
            c = self._cond(cond, B, xs.device)
            if c is None:
                c = torch.zeros((B, self.block_size_cond), dtype=torch.long, device=xs.device)
            return self._on_side_stream(xs.device, lambda: (eng.forward_onepass if one_pass else eng.forward)(codes, c, cbs))
        return self.teacher_forced_logits(xs, model_aux, cond, amp=amp)

    def _one_pass(self):
        if self.forward_mode not in ('stepped', 'one_pass'):
            raise ValueError(f"forward_mode = {self.forward_mode!r} ('stepped' or 'one_pass')")
        return self.forward_mode == 'one_pass'

    @torch.no_grad()
    def teacher_forced_logits(self, xs, model_aux=None, cond=None, amp=False):
        """seq_logits of forward() (transformers.py:113-188) for any block_size_cond, via the engine's cached path."""
        (B, H, W, D) = xs.shape
        assert torch.Size([H, W, D]) == self.block_size
        self._cf = None
        eng = self._eng(amp)
        cbs = self._checked_codebooks(model_aux)
        codes = xs.to(torch.long).contiguous()
        c = self._cond(cond, B, xs.device)
        if self._one_pass():
            def run():
                out = eng.forward_onepass(codes, c, cbs)
                return out[0] if isinstance(out, tuple) else out
            return self._on_side_stream(xs.device, run)
        return self._on_side_stream(xs.device, lambda: eng.logits(codes, c, cbs))

    @torch.no_grad()
    def log_probs(self, xs, model_aux=None, cond=None, amp=False):
        """log p(code) of every code of `xs` under forward(): (B,H,W,D) fp32 = log_softmax(forward(xs))[..., xs], or (seq_logp,
        cond_logp (B, block_size_cond-1) = log p(cond[t+1] | cond[:t+1])) when block_size_cond > 1, mirroring what forward() returns
        there.  Always one pass over all positions; the log-softmax and the gather run on sub-chunks of logits rows inside the
        engine, so (B,H,W,D,V) is never allocated: -log_probs(xs).mean() is compute_loss(forward(xs), xs) at any batch size."""
        (B, H, W, D) = xs.shape
        assert torch.Size([H, W, D]) == self.block_size
        self._cf = None
        eng = self._eng(amp)
        cbs = self._checked_codebooks(model_aux)
        codes = xs.to(torch.long).contiguous()
        c = self._cond(cond, B, xs.device)
        if c is None and self.block_size_cond > 1:
            raise ValueError('log_probs of a text-conditioned model needs cond (its tokens are the targets of cond_logp)')
        return self._on_side_stream(xs.device, lambda: eng.log_probs(codes, c, cbs))

    @torch.no_grad()
    def soft_target_loss(self, xs, model_aux=None, cond=None, amp=False, *, soft_targets=None, z_e=None, temp=1.0):
        """The soft-target cross entropy of every code of `xs` under forward(): (B,H,W,D) fp32 =
        soft_target_cross_entropy(forward(xs), soft, reduction='none') (rqvae/optimizer/loss.py:68-84), or (that, cond_logp) when
        block_size_cond > 1, mirroring log_probs.  .mean() is compute_loss(forward(xs), soft, use_soft_target=True) and .mean((0, 1, 2))
        compute_codebook_loss(...) (transformers.py:371-410) -- the way the reference trains and validates stage 2 -- at any batch
        size: the loss is reduced from sub-chunks of logits rows inside the engine, (B,H,W,D,V) logits are never allocated.
        Exactly one of (keyword-only)
          soft_targets (B,H,W,D,V): the soft codes of model_aux.get_soft_codes(...) that came with `xs`, or any weights;
          z_e (B,h,w,embed_dim): the encoder features `xs` was quantised from, with `temp` -- the soft codes of get_soft_codes(temp=temp)
            are formed inside the engine from the residual of the GIVEN codes (argmin or stochastic draws) and never stored.
        All depths must share one vocabulary (NotImplementedError otherwise, as get_soft_codes refuses ragged codebooks)."""
        (B, H, W, D) = xs.shape
        assert torch.Size([H, W, D]) == self.block_size
        self._cf = None
        if (soft_targets is None) == (z_e is None):
            raise ValueError('soft_target_loss: exactly one of soft_targets and z_e must be given')
        eng = self._eng(amp)
        codes = xs.to(torch.long).contiguous()
        c = self._cond(cond, B, xs.device)
        if c is None and self.block_size_cond > 1:
            raise ValueError('soft_target_loss of a text-conditioned model needs cond (its tokens are the targets of cond_logp)')
        V = max(self.vocab_size)
        if soft_targets is not None:
            if tuple(soft_targets.shape) != (B, H, W, D, V):
                raise ValueError(f'soft_targets of shape {tuple(soft_targets.shape)}; expected {(B, H, W, D, V)}')
            cbs = self._checked_codebooks(model_aux)
            soft = soft_targets.detach().to(device=xs.device, dtype=torch.float32).contiguous()
            return self._on_side_stream(xs.device, lambda: eng.soft_loss(codes, c, cbs, soft_targets=soft))
        if not (float(temp) > 0):
            raise ValueError(f'soft_target_loss: temp = {temp} must be > 0')
        quantizer = self._quantizer(model_aux)
        cbs, norms = quantizer.codebook_list()[:D], quantizer._norm_list()[:D]
        z = quantizer.to_code_shape(z_e.detach()).to(device=xs.device, dtype=torch.float32).contiguous()
        return self._on_side_stream(xs.device, lambda: eng.soft_loss(codes, c, cbs, z=z, norms=norms, temp=float(temp)))

    @staticmethod
    def _quantizer(model_aux):
        if model_aux is None or not hasattr(model_aux, 'quantizer'):
            raise ValueError('soft_target_loss(z_e=...) needs model_aux, the RQVAE whose quantiser produced the codes')
        return model_aux.quantizer

    @_truncation_keywords
    @_shared_prompt
    @_anchored
    @torch.no_grad()
    def sample(self, partial_sample, model_aux=None, cond=None, start_loc=(0, 0), temperature=1.0, top_k=None, top_p=None,
               amp=False, cached=True, is_tqdm=False, desc="Sampling", fast=True, *, keep_mask=None):
        """transformers.py:294-369.  ``keep_mask`` (not in the reference; keyword-only): codes of `partial_sample` to hold fixed --
        (B,H,W,D), (B,H,W), (H,W,D) or (H,W), bool or integer (nonzero = kept); a mask without D applies to every depth, one without B
        to every image.  A kept code stays as given and conditions everything drawn after it; every other code is drawn exactly as
        the unmasked call draws it (same logits, filter and Philox counter), whatever `partial_sample` holds there.  Positions before
        `start_loc` are kept in addition.  Inpainting, outpainting, depth refinement and a region per image are masks; None: the
        reference's behaviour.
        Per-image parameters (not in the reference): ``temperature`` as a (B,) tensor, ``top_k`` / ``top_p`` as (B,) or (B, D) tensors
        give every image its own values (numbers and lists keep the reference's meaning: one value, or one per depth, for every
        image; arguments not given as tensors are broadcast).  Image b is drawn exactly as a call with b's values as scalars draws
        row b, whatever the other images ask for, and one set of captured graphs serves every setting.  Inside ``with
        self.seeds(s)`` image b draws from the Philox stream of seed s[b] instead of the device generator (see seeds()).
        Inside ``with self.return_log_probs():`` the call returns ``(codes, SampleLogProbs(draw, model, None))`` -- the codes are those
        of the plain call (see return_log_probs()).
        ``self.prefix_mode = 'one_pass'``: the given leading positions (before `start_loc`, or a leading run kept in every image) fill
        the KV cache in one pass instead of one step each (see __init__); the codes then differ from the stepped mode's wherever a draw
        was close -- GEMM tiles differ, filters and Philox counters are the same.
        ``min_p=`` / ``typical_p=`` (not in the reference; keywords, or ``with self.truncation(min_p=..., typical_p=...)`` around the
        call: see truncation()): min-p and locally typical sampling after top-p."""
        assert self.block_size == partial_sample.shape[1:]
        if self._extra_conds is not None:
            raise NotImplementedError('extra_conds() composes guidance: it needs sample_guided() (an unguided call has no pair to fold into)')
        self._cf = None
        (H, W, D) = self.block_size
        if self._schedule:
            return self._sample_scheduled(partial_sample, model_aux, cond, start_loc, temperature, top_k, top_p, amp, cached, keep_mask)
        want = self._want_log_probs(cached)
        trunc, force_rows = self._trunc_args(partial_sample.shape[0], *self._truncation)
        rows = self._per_image(partial_sample.shape[0], temperature, top_k, top_p, force=force_rows)
        if rows is not None:
            return self._sample_per_image(rows, partial_sample, model_aux, cond, start_loc, amp, cached, keep_mask, want_logp=want, trunc=trunc)
        top_k_list, top_p_list = self._filter_lists(top_k, top_p)
        B = partial_sample.shape[0]
        device = partial_sample.device
        eng = self._sampling_eng(amp)                   # amp=True: the fp16 build of the engine (the reference's fp16 autocast)
        cbs = self._checked_codebooks(model_aux)
        xs = partial_sample.to(torch.long).contiguous()
        c = self._cond(cond, B, device)
        keep, active = (None, None) if keep_mask is None else self._keep_flags(keep_mask, xs, start_loc)
        if keep is not None and (self.sampler == 'torch' or not cached):
            # the host loops run teacher-forced passes over the whole map, which embed every code: what `partial_sample` holds at a
            # code to be drawn is never used, but it has to be a code (the engine's masked entry point never reads it)
            xs = torch.where(keep, xs, torch.zeros_like(xs))
        if self.sampler == 'torch':
            if not cached:
                raise NotImplementedError("sampler='torch' steps the cached engine; cached=False is available with the default sampler")
            return self._sample_torch_multinomial(eng, xs, c, cbs, start_loc, temperature, top_k_list, top_p_list, keep, active)
        seed, offset = self._draw_rng(device, H * W * D)
        if not cached:
            return self._sample_uncached(eng, xs, c, cbs, start_loc, temperature, top_k_list, top_p_list, seed, offset, keep, active, trunc=trunc)
        tr = self._trunc_engine(trunc)

        def armed(call):                                 # (the arming and the call on the same stream attempt)
            def run():
                if not tr:
                    return call()
                eng.arm_trunc(*tr)
                try:
                    return call()
                finally:
                    eng.arm_trunc(None, None)        # (a call refused before it reached the library leaves nothing armed)
            return run
        if keep is not None:
            keep8 = keep.to(torch.uint8).contiguous()
            pos_active = [bool(a) for a in active.any(dim=1).tolist()]
            return self._with_log_probs(want, self._on_side_stream(device, armed(lambda: eng.sample_masked(
                xs, keep8, pos_active, c, cbs, temperature, top_k_list, top_p_list, seed, offset, self.use_graph, **want))))
        out = self._on_side_stream(device, armed(lambda: eng.sample(xs, c, cbs, start_loc, temperature, top_k_list, top_p_list,
                                                                    seed, offset, self.use_graph, **want)))
        return self._with_log_probs(want, out)

    @contextlib.contextmanager
    def return_log_probs(self, on=True):
        """Log-probabilities of the draws (not in the reference).  The sample() / sample_guided() calls made inside the block return
        ``(codes, SampleLogProbs(draw, model, model_uncond))`` instead of ``codes``; the codes are bit for bit those of the same call
        outside the block.  (B,H,W,D) fp32 each: ``draw`` the log of the probability the drawn code had in the distribution it was
        drawn from (logits after guidance, temperature, top-k, top-p and renormalisation; +0.0 for kept codes and codes before
        start_loc), ``model`` log_softmax of the image's raw conditional logits at the code (kept codes included; NaN where no head
        ran: before start_loc, fully kept positions), ``model_uncond`` the same under `uncond` (None for sample()).  Works with scalar
        and per-image parameters, seeds(), keep_mask, start_loc, amp and use_graph on or off; the host loops (``sampler='torch'``,
        ``cached=False``) return codes only and raise NotImplementedError inside the block.  (A context rather than an argument, like
        seeds() and for its reason: the argument lists of sample() and sample_guided() stay as they are.)"""
        saved, self._return_log_probs = self._return_log_probs, bool(on)
        try:
            yield self
        finally:
            self._return_log_probs = saved

    def _want_log_probs(self, cached):
        """keyword arguments of the engine's sampling calls inside return_log_probs() (none outside); the host loops have no such path"""
        if not self._return_log_probs:
            return {}
        if self.sampler == 'torch' or not cached:
            raise NotImplementedError("return_log_probs() needs the engine's own sampling loop: log-probabilities are not available with "
                                      "sampler='torch' or cached=False (the host loops return codes only)")
        return dict(want_logp=True)

    @staticmethod
    def _with_log_probs(want, result):
        if not want:
            return result
        codes, lp = result
        return codes, SampleLogProbs(*lp)

    @contextlib.contextmanager
    def truncation(self, min_p=None, typical_p=None):
        """Min-p and locally typical sampling (not in the reference) for the sample() / sample_guided() calls made inside the block --
        or pass ``min_p=`` / ``typical_p=`` to those calls as keywords, which is the same.  Two more truncation rules, applied after
        top-p, each to the renormalised output of the stage before it: min-p (0 < min_p <= 1) drops every code whose probability is
        below min_p times the leader's; locally typical sampling (0 <= typical_p < 1) keeps the codes whose surprisal is closest to
        the entropy of the distribution, in that order (ties: lowest code first), up to and including the first whose cumulative
        mass reaches typical_p.  Each a float, a sequence of D per-depth values, or a (B,) / (B, D) tensor, which makes the call a
        per-image call as a top_p tensor does: image b is drawn as the scalar call with b's values draws it.  None, min_p <= 0 and
        typical_p >= 1 (or < 0) are off: the plain call, bit for bit.  Everything runs inside the engine and composes with keep_mask,
        start_loc, seeds(), return_log_probs() (draw: the log-probability after all stages), guidance, amp and prefix_mode;
        ``cached=False`` returns the cached call's codes; ``sampler='torch'`` raises NotImplementedError."""
        saved, self._truncation = self._truncation, (min_p, typical_p)
        try:
            yield self
        finally:
            self._truncation = saved

    def _trunc_args(self, B, min_p, typical_p):
        """min_p / typical_p of sample() -> (None when both are off everywhere, else dict(mp=, ty=, per_image=): D values each -- or,
        per_image, B rows of D -- with the off values 0.0 / -1.0 where a filter is off; is one of them a tensor (a per-image call)?)"""
        D = self.block_size[2]

        def per(a):
            return torch.is_tensor(a) and a.dim() >= 1
        per_image = per(min_p) or per(typical_p)
        if min_p is None and typical_p is None:
            return None, False
        if self.sampler == 'torch':
            raise NotImplementedError("min_p / typical_p are filters of the on-device sampler; sampler='torch' draws with torch.multinomial "
                                      "from the reference's two filters")

        def values(a, name, off):
            if a is None:
                v = [[off] * D]
            elif per(a):
                if a.dim() not in (1, 2) or a.shape[0] != B or (a.dim() == 2 and a.shape[1] != D) or not a.dtype.is_floating_point:
                    raise ValueError(f'{name} of shape {tuple(a.shape)} / {a.dtype}; expected a floating-point ({B},) or ({B}, {D}) tensor')
                v = (a if a.dim() == 2 else a[:, None].expand(B, D)).to(torch.float32).tolist()
            elif isinstance(a, (int, float)) or (torch.is_tensor(a) and a.dim() == 0):
                v = [[float(a)] * D]
            else:
                a = [float(x) for x in a]
                if len(a) not in (1, D):
                    raise ValueError(f'{name} with {len(a)} values; expected one, or one per depth ({D})')
                v = [a * D if len(a) == 1 else a]
            if any(not math.isfinite(x) for row in v for x in row):
                raise ValueError(f'{name} holds a non-finite value')
            return v
        mp, ty = values(min_p, 'min_p', 0.0), values(typical_p, 'typical_p', -1.0)
        if any(x > 1.0 for row in mp for x in row):
            raise ValueError('min_p must be at most 1')
        mp = [[x if x > 0.0 else 0.0 for x in row] for row in mp]
        ty = [[x if 0.0 <= x < 1.0 else -1.0 for x in row] for row in ty]
        if not any(x > 0.0 for row in mp for x in row) and not any(x >= 0.0 for row in ty for x in row):
            return None, per_image
        if per_image:
            mp, ty = (m * B if len(m) == 1 else m for m in (mp, ty))
            return dict(mp=mp, ty=ty, per_image=True), True
        return dict(mp=mp[0], ty=ty[0], per_image=False), False

    @staticmethod
    def _trunc_engine(trunc):
        """the arguments of RqtEngine.arm_trunc (None without a filter): D values each, or B * D image-major of a per-image call"""
        if trunc is None:
            return None
        if trunc['per_image']:
            return [x for row in trunc['mp'] for x in row], [x for row in trunc['ty'] for x in row], True
        return trunc['mp'], trunc['ty'], False

    @staticmethod
    def _trunc_on_device(trunc, B, D, device):
        """min_p / typical_p as the per-depth (B,) device tensors of _native.sample_logits_trunc (host loops with per-image tables)"""
        mp = trunc['mp'] if trunc['per_image'] else [trunc['mp']] * B
        ty = trunc['ty'] if trunc['per_image'] else [trunc['ty']] * B
        return ([torch.tensor([r[d] for r in mp], dtype=torch.float32, device=device) for d in range(D)],
                [torch.tensor([r[d] for r in ty], dtype=torch.float32, device=device) for d in range(D)])

    def _filter_lists(self, top_k, top_p):
        """top_k / top_p of sample() -> one value per depth (transformers.py:309-323)"""
        D = self.block_size[2]
        if top_k is None:
            top_k_list = [self.vocab_size[i] for i in range(D)]
        elif isinstance(top_k, int):
            top_k_list = [min(top_k, self.vocab_size[i]) for i in range(D)]
        elif len(top_k) == 1:
            top_k_list = [min(top_k[0], self.vocab_size[i]) for i in range(D)]
        else:
            top_k_list = [min(top_k[i], self.vocab_size[i]) for i in range(D)]
        if top_p is None:
            top_p_list = [1.0 for _ in range(D)]
        elif isinstance(top_p, float):
            top_p_list = [min(top_p, 1.0) for _ in range(D)]
        elif len(top_p) == 1:
            top_p_list = [min(top_p[0], 1.0) for _ in range(D)]
        else:
            top_p_list = [min(top_p[i], 1.0) for i in range(D)]
        return top_k_list, top_p_list

    # ------------------------------------------------------------------ composed guidance
    MAX_EXTRA_CONDS = _native.MAX_EXTRA_CONDS

    @contextlib.contextmanager
    def extra_conds(self, conds, weights):
        """Composed guidance (not in the reference): negative prompts and extra conditions for the sample_guided() calls made inside the
        block.  ``conds``: 1 .. 4 conditionings with the shape and dtype rules of ``cond`` (None = zeros); ``weights``: as many finite
        floats or (B,) tensors (a weight per image).  With c, u and x_k the raw logits of an image under ``cond``, ``uncond`` and
        ``conds[k]``, every code is drawn from

            G = u + s (c - u) + sum_k w_k (x_k - u)

        so a negative prompt is an extra condition with w < 0 (``sample_guided(..., negative=n, negative_scale=w)`` is sugar for
        ``conds=[n], weights=[-w]``) and a second prompt or a style condition one with w > 0.  The loop runs inside the engine over
        (2 + K) B rows (rqamd_rqt_sample_compose): every block sees exactly the codes that were drawn, and filters, temperature and
        Philox counters are those of sample_guided().  All weights zero -- or every extra condition equal to ``uncond`` -- draws what
        the guided call over the same rows draws, bit for bit.  Composes with keep_mask, start_loc, seeds(), per-image parameter
        tensors, truncation(), schedule() (a guidance schedule applies to s; the weights have no schedule), return_log_probs() (draw
        under the composed distribution, model / model_uncond raw as without extra conditions), amp and prefix_mode; ``cached=False``
        is the host loop over the (2 + K) B rows, bit for bit equal to ``cached=True``.  sample(), shared_cond() and ``sampler='torch'``
        raise NotImplementedError inside the block; a different number of conds and weights, more than 4 of them, a wrong shape or a
        non-finite weight raise ValueError before anything runs."""
        conds, weights = list(conds), list(weights)
        if len(conds) != len(weights):
            raise ValueError(f'extra_conds: {len(conds)} conds and {len(weights)} weights')
        if not 1 <= len(conds) <= self.MAX_EXTRA_CONDS:
            raise ValueError(f'extra_conds: {len(conds)} extra conditions; expected 1 .. {self.MAX_EXTRA_CONDS}')
        for w in weights:
            if torch.is_tensor(w):
                if w.dim() > 1 or w.dtype.is_complex or w.dtype == torch.bool or not bool(torch.isfinite(w.to(torch.float32)).all()):
                    raise ValueError(f'extra_conds: weight of shape {tuple(w.shape)} / {w.dtype}; expected finite real values, a number or a (B,) tensor')
            elif not isinstance(w, (int, float)) or isinstance(w, bool) or not math.isfinite(float(w)):
                raise ValueError(f'extra_conds: weight {w!r}; expected a finite number or a (B,) tensor')
        saved, self._extra_conds = self._extra_conds, (conds, weights)
        try:
            yield self
        finally:
            self._extra_conds = saved

    def _compose_args(self, B, device):
        """self._extra_conds for B images, checked -> None outside extra_conds(), else dict(K=, conds= K (B, block_size_cond) int64 tensors
        on `device` or None, w= K rows of B floats on the host)"""
        if self._extra_conds is None:
            return None
        conds, weights = self._extra_conds
        cs, ws = [], []
        for k, c in enumerate(conds):
            if c is not None and (not torch.is_tensor(c) or c.shape[0] != B or c.numel() != B * self.block_size_cond):
                shape = tuple(c.shape) if torch.is_tensor(c) else type(c).__name__
                raise ValueError(f'extra_conds: conds[{k}] of shape {shape}; expected {(B, self.block_size_cond)} (the shape of cond)')
            cs.append(self._cond(c, B, device))
        for k, w in enumerate(weights):
            if torch.is_tensor(w) and w.dim() == 1:
                if w.shape[0] != B:
                    raise ValueError(f'extra_conds: weights[{k}] of shape {tuple(w.shape)}; expected ({B},) (one weight per image)')
                ws.append([float(v) for v in w.to(torch.float32).tolist()])
            else:
                ws.append([float(w)] * B)
        return dict(K=len(cs), conds=cs, w=ws)

    @staticmethod
    def _compose_flat(comp):
        """the arguments of RqtEngine.arm_compose (conds, K * B weights condition-major)"""
        return comp['conds'], [v for row in comp['w'] for v in row]

    def _compose_rows_cat(self, comp, xs, c, u):
        """the (2 + K) B rows of the host loops: codes repeated, conditionings cond, uncond, extras (None where every block is zeros)"""
        B = xs.shape[0]
        blocks = [c, u] + comp['conds']
        c2 = None
        if any(b is not None for b in blocks):
            zeros = torch.zeros((B, self.block_size_cond), dtype=torch.long, device=xs.device)
            c2 = torch.cat([zeros if b is None else b for b in blocks])
        return torch.cat([xs] * len(blocks)), c2

    @staticmethod
    def _compose_rows(logits, n, comp, scales):
        """compose_logits over the (2 + K) blocks of n rows of `logits`, with one scale (a float) or one per row (a list): the rows of each
        distinct scale through the entry point -- elementwise, so row b is what the engine's fold and guided sampler mix for b"""
        K = comp['K']
        W = torch.tensor(comp['w'], dtype=torch.float32, device=logits.device)
        cu, x = logits[:2 * n], logits[2 * n:].reshape(K, n, -1)
        if not isinstance(scales, (list, tuple)):
            return _native.compose_logits(cu[:n], cu[n:], x, W, scales)
        out = torch.empty_like(cu[:n])
        for s in sorted(set(scales)):
            idx = torch.tensor([i for i, v in enumerate(scales) if v == s], dtype=torch.long, device=logits.device)
            out[idx] = _native.compose_logits(cu[:n][idx], cu[n:][idx], x[:, idx], W[:, idx], s)
        return out

    # ------------------------------------------------------------------ anchored sampling
    @contextlib.contextmanager
    def anchor(self, z, weight=1.0):
        """Anchored sampling (not in the reference): the sample() / sample_guided() calls made inside the block draw codes near an encoded
        image -- variations of an image, img2img with a strength knob, soft inpainting.  ``z``: the output of ``model_aux.encode(images)``,
        (B, H, W, input_embed_dim) fp32; None is the plain call.  At every step the logits of image b get the quantiser's own soft-code
        term for the residual the image has at that depth given the codes drawn so far,

            x'[v] = x[v] - w(b, p, d) * dist(r_d(b, p), codebook_d[v]),    r_0 = z[b, p],   r_{d+1} = r_d - codebook_d[code(b, p, d)]

        with dist the quantiser's squared distance in fp32: w = 0 is the prior, w -> inf is ``model_aux.get_codes(images)``, and in
        between every code is drawn from p_model * softmax(-dist / temp) with w = 1 / temp, ``get_soft_codes`` used as a likelihood.
        ``weight`` (>= 0, finite): a float; a sequence of D per-depth values (keep the layout -- depth 0 or 1 -- and redraw the detail,
        or the reverse); or a tensor of shape (B,), (B, D), (H, W) (a soft inpainting mask), (H, W, D) or (B, H, W, D).  Codebooks and
        norms come from ``model_aux``, as for soft_target_loss(z_e=...).  The loop runs inside the engine (rqamd_rqt_sample_anchor): three
        more launches per step, captured graphs of their own whose keys hold no z and no weight; filters, temperature and Philox
        counters are those of the plain call, and weight 0 returns its codes bit for bit.  An image whose z holds a NaN or an inf
        degrades to unanchored.  Composes with keep_mask (the residual follows the kept code), start_loc, prefix_mode / kept_run_mode,
        per-image tensors, seeds(), truncation(), schedule(), guidance, amp and return_log_probs() (draw: under the anchored
        distribution after all stages; model / model_uncond: the raw logits); ``cached=False`` is the host loop over
        _native.anchor_logits, bit for bit equal to ``cached=True``.  shared_cond(), extra_conds(), ``sampler='torch'``, depths with
        different vocabularies and a z width other than 64 / 128 / 192 / 256 raise NotImplementedError; a wrong shape or a negative or
        non-finite weight raises ValueError, before anything runs."""
        saved, self._anchor = self._anchor, None if z is None else (z, weight)
        try:
            yield self
        finally:
            self._anchor = saved

    def _anchor_args(self, partial_sample, model_aux):
        """self._anchor for the images of `partial_sample`, checked -> dict(z= (B, H, W, dim) fp32 on the device, cbs= / norms= D tensors,
        w= (1 or B, H*W, D) fp32 on the host, per_image=, w_dev= (B, H*W, D) on the device for the host loops)"""
        z, weight = self._anchor
        (H, W, D) = self.block_size
        B, device = partial_sample.shape[0], partial_sample.device
        if self.sampler == 'torch':
            raise NotImplementedError("anchor() runs in the on-device sampler; sampler='torch' has no anchored form")
        if self._shared_cond:
            raise NotImplementedError('anchor() inside shared_cond(): rqamd_rqt_sample_anchor together with rqamd_rqt_sample_shared is not built')
        if self._extra_conds is not None:
            raise NotImplementedError('anchor() inside extra_conds(): rqamd_rqt_sample_anchor together with rqamd_rqt_sample_compose is not built')
        V = max(self.vocab_size)
        if any(v != V for v in self.vocab_size):
            raise NotImplementedError(f'anchor(): depths with different vocabularies ({list(self.vocab_size)}); one codebook size is needed')
        if model_aux is None or not hasattr(model_aux, 'quantizer'):
            raise ValueError('anchor() needs model_aux, the RQVAE whose encoder produced z and whose quantiser holds the codebooks')
        quantizer = model_aux.quantizer
        if not torch.is_tensor(z) or z.dim() != 4:
            raise ValueError(f'anchor: z of shape {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}; expected ({B}, {H}, {W}, dim)')
        try:
            z = quantizer.to_code_shape(z.detach()).to(device=device, dtype=torch.float32).contiguous()
        except RuntimeError:
            raise ValueError(f'anchor: z of shape {tuple(z.shape)} does not fold into the code shape ({B}, {H}, {W}, dim)') from None
        if tuple(z.shape[:3]) != (B, H, W):
            raise ValueError(f'anchor: z of shape {tuple(z.shape)}; expected ({B}, {H}, {W}, dim)')
        dim = z.shape[3]
        if dim not in _native.ANCHOR_DIMS:
            raise NotImplementedError(f'anchor: dim {dim} must be 64, 128, 192 or 256')
        cbs, norms = quantizer.codebook_list()[:D], quantizer._norm_list()[:D]
        if len(cbs) < D:
            raise ValueError(f'model_aux has {len(cbs)} codebooks, the transformer needs {D}')
        for d, cb in enumerate(cbs):
            if tuple(cb.shape) != (V, dim):
                raise ValueError(f'anchor: codebook {d} has shape {tuple(cb.shape)}; expected ({V}, {dim})')
        if torch.is_tensor(weight):
            t = weight.detach().cpu()
            if t.dtype.is_complex or t.dtype == torch.bool:
                raise ValueError(f'anchor: weight of dtype {t.dtype}; expected real values')
            t, shp = t.to(torch.float32), tuple(weight.shape)
            forms = {(): (1, 1, 1), (B,): (B, 1, 1), (B, D): (B, 1, D), (H, W): (1, H * W, 1), (H, W, D): (1, H * W, D), (B, H, W, D): (B, H * W, D)}
            if shp not in forms:
                raise ValueError(f'anchor: weight of shape {shp}; expected {(B,)}, {(B, D)}, {(H, W)}, {(H, W, D)} or {(B, H, W, D)}')
            if (B, D) == (H, W) and shp == (B, D):
                raise ValueError(f'anchor: weight of shape {shp} is both (B, D) and (H, W) here; pass it as {(B, H, W, D)}')
            t = t.reshape(forms[shp])
        elif isinstance(weight, (int, float)) and not isinstance(weight, bool):
            t = torch.full((1, 1, 1), float(weight), dtype=torch.float32)
        else:
            vals = [float(v) for v in weight]
            if len(vals) != D:
                raise ValueError(f'anchor: {len(vals)} weights; expected a number, one value per depth ({D}) or a tensor')
            t = torch.tensor(vals, dtype=torch.float32).reshape(1, 1, D)
        if not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
            raise ValueError('anchor: every weight must be finite and >= 0')
        per_image = t.shape[0] > 1
        w = t.expand(B if per_image else 1, H * W, D).contiguous()
        return dict(z=z, cbs=cbs, norms=norms, w=w, per_image=per_image, w_dev=w.expand(B, H * W, D).to(device))

    def _anchor_step(self, logits, xs, n, pos, d, guided):
        """host loops: the logits of step (pos, d) with the anchor of this call folded in (_native.anchor_logits: the engine's three
        launches over the n images) -- both halves of a guided step; unchanged outside anchor()"""
        a = self._anchor_live
        if a is None:
            return logits
        h, w = divmod(pos, self.block_size[1])
        z_rows, codes, wt = a['z'][:, h, w], xs[:n, h, w, :d], a['w_dev'][:, pos, d]
        if guided:
            return torch.cat(_native.anchor_logits(logits[:n], z_rows, codes, a['cbs'], a['norms'], wt, logits_u=logits[n:2 * n]))
        return _native.anchor_logits(logits, z_rows, codes, a['cbs'], a['norms'], wt)

    # ------------------------------------------------------------------ per-image sampling parameters
    @contextlib.contextmanager
    def shared_cond(self, n):
        """Shared-prompt sampling (not in the reference's model; its notebooks repeat one tokenised prompt num_samples times): the
        sample() / sample_guided() calls made inside the block draw ``n`` images per prompt.  ``partial_sample`` has G * n rows, ``cond``
        (and ``uncond``) G rows; image r belongs to prompt r // n.  Image r is drawn exactly as the plain call with
        ``cond.repeat_interleave(n, 0)`` draws it -- same kernels, filters, Philox key and counters -- but the text prefix of a prompt
        goes through the body stack once, its keys and values are cached once, and the decode attention reads that one copy for the n
        images (rqamd_rqt_sample_shared).  The codes equal the plain call's bit for bit wherever the prefill over G prompts and the
        prefill over G * n rows fall into one GEMM regime, and differ only where a draw was close elsewhere, as with prefix_mode.
        Text-conditioned models (block_size_cond >= 2) with body head size 64, a body context of at most 256 tokens and the default
        cache format.  Composes with keep_mask, start_loc, seeds(), return_log_probs(), truncation(), schedule(), amp and per-image
        tensors (B = G * n values); a code prefix is stepped whatever prefix_mode says.  ``sampler='torch'`` and ``cached=False`` raise
        NotImplementedError, a ``cond`` / ``uncond`` of another shape ValueError.  n = 1 is allowed and runs the shared path.
        The engine's KV workspace has one layout at a time: the first shared call after a plain one (and the other way round) lays
        it out again and recaptures its graphs."""
        n = int(n)
        if n < 1:
            raise ValueError(f'shared_cond({n}): n must be >= 1')
        saved, self._shared_cond = self._shared_cond, n
        try:
            yield self
        finally:
            self._shared_cond = saved

    @contextlib.contextmanager
    def seeds(self, seeds):
        """Per-image Philox seeds for the sample() / sample_guided() calls made inside the block: ``seeds`` is a (B,) integer tensor
        or a sequence of B non-negative integers.  Image b is then drawn from the stream of row 0 of a call made after
        ``torch.manual_seed(seeds[b])`` -- whatever its place in the batch and whatever the other images are -- and the device
        generator is not consumed.  (A context rather than an argument: the argument lists of sample() and sample_guided() are the
        reference's plus keep_mask / uncond / guidance_scale, and stay so.)  ``sampler='torch'`` has no per-row key and raises."""
        if torch.is_tensor(seeds):
            if seeds.dtype.is_floating_point or seeds.dtype.is_complex or seeds.dtype == torch.bool or seeds.dim() != 1:
                raise ValueError(f'seeds of shape {tuple(seeds.shape)} / {seeds.dtype}; expected a (B,) integer tensor')
            vals = [int(v) for v in seeds.tolist()]
        else:
            vals = list(seeds)
            if not all(isinstance(v, int) and not isinstance(v, bool) for v in vals):
                raise ValueError('seeds must be integers')
        if any(v < 0 or v >= 2 ** 64 for v in vals):
            raise ValueError('seeds must be in 0 .. 2**64 - 1 (negative seeds are refused)')
        saved, self._image_seeds = self._image_seeds, vals
        try:
            yield self
        finally:
            self._image_seeds = saved

    def _per_image(self, B, temperature, top_k, top_p, guidance_scale=None, force=False):
        """None when no argument is per image (no tensor of one or more dimensions, no seeds(): the scalar entry points, untouched), else
        the per-image tables on the host, validated: T [B], tk / tp [B][D] (clipped like _filter_lists: top_k to vocab_size[d], top_p
        to 1.0), gs [B] or None, seeds [B] or None"""
        def per(a):
            return torch.is_tensor(a) and a.dim() >= 1
        if not (force or per(temperature) or per(top_k) or per(top_p) or per(guidance_scale) or self._image_seeds is not None):
            return None                                  # (force: min_p / typical_p came as tensors)
        D = self.block_size[2]

        def vec(a, name, default):
            if per(a):
                if tuple(a.shape) != (B,):
                    raise ValueError(f'{name} of shape {tuple(a.shape)}; expected ({B},) (one value per image)')
                if a.dtype.is_complex or a.dtype == torch.bool:
                    raise ValueError(f'{name} of dtype {a.dtype}; expected a real tensor')
                return [float(v) for v in a.to(torch.float32).tolist()]
            return [float(default if a is None else a)] * B

        def table(a, name, integer):
            if a.dim() not in (1, 2) or a.shape[0] != B or (a.dim() == 2 and a.shape[1] != D):
                raise ValueError(f'{name} of shape {tuple(a.shape)}; expected ({B},) or ({B}, {D})')
            if integer and (a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool):
                raise ValueError(f'{name} of dtype {a.dtype}; expected an integer tensor')
            if not integer and not a.dtype.is_floating_point:
                raise ValueError(f'{name} of dtype {a.dtype}; expected a floating-point tensor')
            a = a if a.dim() == 2 else a[:, None].expand(B, D)
            return (a if integer else a.to(torch.float32)).tolist()
        top_k_list, top_p_list = self._filter_lists(None if per(top_k) else top_k, None if per(top_p) else top_p)
        tk = [list(top_k_list) for _ in range(B)]
        tp = [list(top_p_list) for _ in range(B)]
        if per(top_k):
            tk = [[min(int(k), self.vocab_size[d]) for d, k in enumerate(row)] for row in table(top_k, 'top_k', True)]
        if per(top_p):
            tp = [[min(float(p), 1.0) for p in row] for row in table(top_p, 'top_p', False)]
            if any(p != p for row in tp for p in row):
                raise ValueError('top_p holds NaN')
        T = vec(temperature, 'temperature', 1.0)
        if not all(math.isfinite(t) and t > 0 for t in T):
            raise ValueError('every temperature must be > 0 and finite')
        gs = None
        if guidance_scale is not None:
            gs = vec(guidance_scale, 'guidance_scale', 1.0)
            if not all(math.isfinite(s) for s in gs):
                raise ValueError('every guidance_scale must be finite')
        sd = self._image_seeds
        if sd is not None and len(sd) != B:
            raise ValueError(f'seeds of shape ({len(sd)},); expected ({B},) (one seed per image)')
        return dict(T=T, tk=tk, tp=tp, gs=gs, seeds=sd)

    def _rows_on_device(self, rows, device):
        """the tables of _per_image as the device tensors _native.sample_logits_rows takes (host loops): T (B,), tk / tp one (B,) per depth"""
        D = self.block_size[2]
        dev = dict(rows)
        dev['T_dev'] = torch.tensor(rows['T'], dtype=torch.float32, device=device)
        dev['tk_dev'] = [torch.tensor([r[d] for r in rows['tk']], dtype=torch.int32, device=device) for d in range(D)]
        dev['tp_dev'] = [torch.tensor([r[d] for r in rows['tp']], dtype=torch.float32, device=device) for d in range(D)]
        sd = rows['seeds']
        dev['seeds_dev'] = None if sd is None else torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in sd], dtype=torch.int64, device=device)
        return dev

    @staticmethod
    def _guide_rows(c, u, scales):
        """guide_logits with one scale per row: the rows of each distinct scale through the scalar entry point (elementwise, so row b
        is what the engine's guided sampler mixes for b)"""
        out = torch.empty_like(c)
        for s in sorted(set(scales)):
            idx = torch.tensor([i for i, v in enumerate(scales) if v == s], dtype=torch.long, device=c.device)
            out[idx] = _native.guide_logits(c[idx].contiguous(), u[idx].contiguous(), s)
        return out

    def _sample_per_image(self, rows, partial_sample, model_aux, cond, start_loc, amp, cached, keep_mask, guided=False, uncond=None,
                          want_logp={}, trunc=None):
        """sample() / sample_guided() with per-image parameters: rqamd_rqt_sample_rows, or the two host loops over sample_logits_rows"""
        (H, W, D) = self.block_size
        B = partial_sample.shape[0]
        device = partial_sample.device
        if guided and uncond is not None and (uncond.shape[0] != self._cond_rows(B) or uncond.numel() != self._cond_rows(B) * self.block_size_cond):
            raise ValueError(f'uncond of shape {tuple(uncond.shape)}; expected {(self._cond_rows(B), self.block_size_cond)} (the shape of cond)')
        if rows['seeds'] is not None and self.sampler == 'torch':
            raise ValueError("sampler='torch' draws with torch.multinomial from the device generator, which has no per-row key: seeds() is "
                             'available with the default sampler')
        if self.sampler == 'torch' and not cached:
            raise NotImplementedError("sampler='torch' steps the cached engine; cached=False is available with the default sampler")
        eng = self._sampling_eng(amp)
        cbs = self._checked_codebooks(model_aux)
        xs = partial_sample.to(torch.long).contiguous()
        c = self._cond(cond, B, device)
        u = self._cond(uncond, B, device) if guided else None
        comp = self._compose_args(B, device) if guided else None
        keep, active = (None, None) if keep_mask is None else self._keep_flags(keep_mask, xs, start_loc)
        if self.sampler == 'torch' or not cached:
            if keep is not None:
                xs = torch.where(keep, xs, torch.zeros_like(xs))            # (see sample(): the host loops embed every code)
            xs2, c2, scale = xs, c, None
            if comp is not None:
                (xs2, c2), scale = self._compose_rows_cat(comp, xs, c, u), rows['gs']
            elif guided:
                xs2, scale = torch.cat([xs, xs]), rows['gs']
                if c is not None or u is not None:
                    zeros = torch.zeros((B, self.block_size_cond), dtype=torch.long, device=device)
                    c2 = torch.cat([zeros if c is None else c, zeros if u is None else u])
            dev = self._rows_on_device(rows, device)
            if self.sampler == 'torch':
                return self._sample_torch_multinomial(eng, xs2, c2, cbs, start_loc, None, None, None, keep, active, scale, rows=dev)
            seed, offset = (0, 0) if rows['seeds'] is not None else self._draw_rng(device, H * W * D)
            return self._sample_uncached(eng, xs2, c2, cbs, start_loc, None, None, None, seed, offset, keep, active, scale, rows=dev, trunc=trunc,
                                         comp=comp)
        seed, offset = (0, 0) if rows['seeds'] is not None else self._draw_rng(device, H * W * D)
        keep8, pos_active, start = None, None, start_loc
        if keep is not None:
            keep8 = keep.to(torch.uint8).contiguous()
            pos_active = [bool(a) for a in active.any(dim=1).tolist()]
            start = (0, 0)                                                   # (the kept prefix is part of `keep`)
        tr = self._trunc_engine(trunc)

        def run():
            if tr:
                eng.arm_trunc(*tr)
            if comp is not None:
                eng.arm_compose(*self._compose_flat(comp))
            try:
                return eng.sample_rows(xs, keep8, pos_active, c, u, cbs, start, rows['T'], rows['tk'], rows['tp'], rows['gs'] if guided else None,
                                       rows['seeds'], seed, offset, self.use_graph, **want_logp)
            finally:
                eng.arm_trunc(None, None)
                eng.arm_compose()
        return self._with_log_probs(want_logp, self._on_side_stream(device, run))

    @_negative_prompt
    @_truncation_keywords
    @_shared_prompt
    @_anchored
    @torch.no_grad()
    def sample_guided(self, partial_sample, model_aux=None, cond=None, start_loc=(0, 0), temperature=1.0, top_k=None, top_p=None,
                      amp=False, cached=True, is_tqdm=False, desc="Sampling", fast=True, *, uncond=None, guidance_scale=1.0,
                      keep_mask=None):
        """sample() with classifier-free guidance (not in the reference): every code is drawn from the guided logits
        g = u + s (c - u), c / u the raw logits of the image under `cond` / under `uncond` (same shape and dtype rules as `cond`;
        None = zeros, as cond=None), s = `guidance_scale` (any finite value; 1: the conditional logits, bit for bit).  The loop runs
        inside the engine over 2B rows (rqamd_rqt_sample_guided): the unconditional twin of an image sees exactly the codes its
        conditional twin drew, and row b uses the temperature, top-k, top-p and Philox counter of row b of sample().  Returns
        (B,H,W,D) int64.  ``keep_mask`` composes as in sample(); ``cached=False`` and ``sampler='torch'`` are the host loops of
        sample() over the 2B rows, the former bit for bit equal to ``cached=True``.  Per-image ``temperature`` / ``top_k`` / ``top_p``
        tensors and ``with self.seeds(...)`` as in sample(); ``guidance_scale`` as a (B,) tensor gives every image its own scale.
        Inside ``with self.return_log_probs():`` the call returns ``(codes, SampleLogProbs(draw, model, model_uncond))``, draw under the
        guided distribution, model / model_uncond under the raw logits of the two twins.  ``min_p`` / ``typical_p`` as in sample(),
        applied to the guided distribution.  ``negative=`` / ``negative_scale=`` (keywords) and ``with self.extra_conds(...)``: negative
        prompts and extra conditions folded into the guided logits (see extra_conds())."""
        assert self.block_size == partial_sample.shape[1:]
        self._cf = None
        (H, W, D) = self.block_size
        if self._schedule:
            return self._sample_scheduled(partial_sample, model_aux, cond, start_loc, temperature, top_k, top_p, amp, cached, keep_mask,
                                          guided=True, uncond=uncond, guidance_scale=guidance_scale)
        want = self._want_log_probs(cached)
        trunc, force_rows = self._trunc_args(partial_sample.shape[0], *self._truncation)
        rows = self._per_image(partial_sample.shape[0], temperature, top_k, top_p, guidance_scale, force=force_rows)
        if rows is not None:
            return self._sample_per_image(rows, partial_sample, model_aux, cond, start_loc, amp, cached, keep_mask, True, uncond, want_logp=want,
                                          trunc=trunc)
        if not math.isfinite(float(guidance_scale)):
            raise ValueError(f'guidance_scale {guidance_scale} is not finite')
        scale = float(guidance_scale)
        top_k_list, top_p_list = self._filter_lists(top_k, top_p)
        B = partial_sample.shape[0]
        device = partial_sample.device
        if uncond is not None and (uncond.shape[0] != self._cond_rows(B) or uncond.numel() != self._cond_rows(B) * self.block_size_cond):
            raise ValueError(f'uncond of shape {tuple(uncond.shape)}; expected {(self._cond_rows(B), self.block_size_cond)} (the shape of cond)')
        eng = self._sampling_eng(amp)
        cbs = self._checked_codebooks(model_aux)
        xs = partial_sample.to(torch.long).contiguous()
        c, u = self._cond(cond, B, device), self._cond(uncond, B, device)
        comp = self._compose_args(B, device)
        keep, active = (None, None) if keep_mask is None else self._keep_flags(keep_mask, xs, start_loc)
        if self.sampler == 'torch' or not cached:
            if self.sampler == 'torch' and not cached:
                raise NotImplementedError("sampler='torch' steps the cached engine; cached=False is available with the default sampler")
            if keep is not None:
                xs = torch.where(keep, xs, torch.zeros_like(xs))            # (see sample(): the host loops embed every code)
            # the host loops run the engine's unguided entry points over the 2B rows themselves: images under cond, then their twins
            # (composed guidance: then the K blocks under the extra conditions)
            xs2 = torch.cat([xs, xs])
            c2 = None
            if comp is not None:
                xs2, c2 = self._compose_rows_cat(comp, xs, c, u)
            elif c is not None or u is not None:
                zeros = torch.zeros((B, self.block_size_cond), dtype=torch.long, device=device)
                c2 = torch.cat([zeros if c is None else c, zeros if u is None else u])
            if self.sampler == 'torch':
                return self._sample_torch_multinomial(eng, xs2, c2, cbs, start_loc, temperature, top_k_list, top_p_list, keep, active, scale)
            seed, offset = self._draw_rng(device, H * W * D)
            return self._sample_uncached(eng, xs2, c2, cbs, start_loc, temperature, top_k_list, top_p_list, seed, offset, keep, active, scale,
                                         trunc=trunc, comp=comp)
        seed, offset = self._draw_rng(device, H * W * D)
        keep8, pos_active, start = None, None, start_loc
        if keep is not None:
            keep8 = keep.to(torch.uint8).contiguous()
            pos_active = [bool(a) for a in active.any(dim=1).tolist()]
            start = (0, 0)                                                   # (the kept prefix is part of `keep`)
        tr = self._trunc_engine(trunc)

        def run():
            if tr:
                eng.arm_trunc(*tr)
            if comp is not None:
                eng.arm_compose(*self._compose_flat(comp))
            try:
                return eng.sample_guided(xs, keep8, pos_active, c, u, cbs, start, temperature, scale, top_k_list, top_p_list, seed, offset,
                                         self.use_graph, **want)
            finally:
                eng.arm_trunc(None, None)
                eng.arm_compose()
        return self._with_log_probs(want, self._on_side_stream(device, run))

    # ------------------------------------------------------------------ sampling schedules over positions and depths
    SCHEDULE_PARAMETERS = ('temperature', 'top_k', 'top_p', 'guidance_scale', 'min_p', 'typical_p')

    @contextlib.contextmanager
    def schedule(self, temperature=None, top_k=None, top_p=None, guidance_scale=None, min_p=None, typical_p=None):
        """Sampling parameters that change along the raster order (not in the reference), for the sample() / sample_guided() calls made
        inside the block: a guidance scale that ramps up over the positions, a temperature that anneals, a tight top-k for the first
        rows, a colder temperature at the deeper codes of some positions.  Each value is a tensor, array or nested list of shape (H, W)
        (every depth of a position alike), (H, W, D), or (B, H, W, D) (a schedule per image), and replaces that parameter of the call:
        passing the call a value other than the default for a scheduled parameter as well is a ValueError, as is a wrong shape, a
        temperature that is not finite and > 0, a non-finite guidance scale / min_p / typical_p or a min_p above 1.  Code (b, h, w, d) is
        drawn exactly as the call that gives every image's values at (b, h, w, d) as per-image values draws it there -- same logits,
        same Philox counter -- so a schedule that is constant over the positions returns the unscheduled call's codes.  top_k / top_p /
        min_p / typical_p use their off values as in the per-image tensors (top_k >= vocab_size, top_p >= 1, min_p <= 0, typical_p >= 1).
        Parameters that are not scheduled keep every form they have (number, per-depth list, per-image tensor).  Everything runs inside
        the engine, on captured graphs whose keys hold no value (another schedule replays them), and composes with keep_mask, start_loc,
        amp, use_graph, prefix_mode, seeds(), return_log_probs() (draw: the log-probability after all stages, with the position's values)
        and truncation(); ``cached=False`` returns the cached call's codes; ``sampler='torch'`` raises NotImplementedError.
        position_ramp() makes the usual ramps.  (A context rather than arguments, like seeds(): the argument lists stay as they are.)"""
        given = dict(temperature=temperature, top_k=top_k, top_p=top_p, guidance_scale=guidance_scale, min_p=min_p, typical_p=typical_p)
        saved, self._schedule = self._schedule, {k: v for k, v in given.items() if v is not None}
        try:
            yield self
        finally:
            self._schedule = saved

    def position_ramp(self, start, end, kind='linear'):
        """(H, W) fp32 tensor that goes from `start` at the first position to `end` at the last one along the raster order: 'linear',
        or 'cosine' (half a cosine period: flat at both ends).  Both end points are exact and the ramp is monotonic."""
        (H, W, _) = self.block_size
        n = H * W
        t = torch.arange(n, dtype=torch.float64) / max(n - 1, 1)
        if kind == 'cosine':
            t = (1.0 - torch.cos(math.pi * t)) / 2.0
        elif kind != 'linear':
            raise ValueError(f"position_ramp: kind = {kind!r} ('linear' or 'cosine')")
        ramp = (float(start) + (float(end) - float(start)) * t).to(torch.float32)
        ramp[0] = float(start)
        if n > 1:
            ramp[-1] = float(end)
        return ramp.view(H, W)

    def _schedule_values(self, B, guided):
        """self._schedule, checked -> ({parameter: (1 or B, H*W, D) tensor on the host, top_k int64 and the others fp32, clipped and with
        the off values of the per-image tables}, is one of them per image?)"""
        (H, W, D) = self.block_size
        out, per_image = {}, False
        for name, v in self._schedule.items():
            t = v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(v)
            if t.dtype.is_complex or t.dtype == torch.bool:
                raise ValueError(f'schedule: {name} of dtype {t.dtype}; expected real values')
            if name == 'top_k':
                if t.dtype.is_floating_point:
                    raise ValueError(f'schedule: top_k of dtype {t.dtype}; expected integers')
                t = t.to(torch.int64)
            else:
                t = t.to(torch.float32)
            shp = tuple(t.shape)
            if shp == (H, W):
                t = t.reshape(1, H * W, 1).expand(1, H * W, D)
            elif shp == (H, W, D):
                t = t.reshape(1, H * W, D)
            elif shp == (B, H, W, D):
                t, per_image = t.reshape(B, H * W, D), True
            else:
                raise ValueError(f'schedule: {name} of shape {shp}; expected {(H, W)}, {(H, W, D)} or {(B, H, W, D)}')
            if name == 'guidance_scale' and not guided:
                raise ValueError('schedule: a guidance_scale schedule needs sample_guided()')
            if name != 'top_k' and not bool(torch.isfinite(t).all()):
                if name != 'top_p' or bool(torch.isnan(t).any()):
                    raise ValueError(f'schedule: {name} holds a non-finite value')
            if name == 'temperature' and not bool((t > 0).all()):
                raise ValueError('schedule: every temperature must be > 0 and finite')
            if name == 'min_p':
                if bool((t > 1.0).any()):
                    raise ValueError('schedule: min_p must be at most 1')
                t = torch.where(t > 0, t, torch.zeros_like(t))
            if name == 'typical_p':
                t = torch.where((t >= 0) & (t < 1.0), t, torch.full_like(t, -1.0))
            if name == 'top_k':
                t = torch.minimum(t, torch.tensor(self.vocab_size, dtype=torch.int64))      # (as _filter_lists: >= vocab_size is off)
            if name == 'top_p':
                t = t.clamp(max=1.0)
            out[name] = t.contiguous()
        return out, per_image

    def _sample_scheduled(self, partial_sample, model_aux, cond, start_loc, temperature, top_k, top_p, amp, cached, keep_mask,
                          guided=False, uncond=None, guidance_scale=1.0):
        """sample() / sample_guided() inside ``with self.schedule(...)``: rqamd_rqt_sample_schedule in front of the entry point the
        unscheduled parameters ask for, or -- cached=False -- the uncached loop over the per-row stand-alone samplers"""
        (H, W, D) = self.block_size
        B = partial_sample.shape[0]
        device = partial_sample.device
        if self.sampler == 'torch':
            raise NotImplementedError("schedule() runs in the on-device sampler; sampler='torch' draws with torch.multinomial from one set "
                                      'of values per call')
        want = self._want_log_probs(cached)
        sched, sched_per_image = self._schedule_values(B, guided)
        min_p, typical_p = self._truncation
        call = dict(temperature=(temperature, lambda v: isinstance(v, (int, float)) and float(v) == 1.0), top_k=(top_k, lambda v: v is None),
                    top_p=(top_p, lambda v: v is None), min_p=(min_p, lambda v: v is None), typical_p=(typical_p, lambda v: v is None),
                    guidance_scale=(guidance_scale, lambda v: isinstance(v, (int, float)) and float(v) == 1.0))
        for name in sched:
            value, is_default = call[name]
            if not is_default(value):
                raise ValueError(f'{name} is scheduled (schedule()) and given to the call as well')
        if 'min_p' in sched:
            min_p = None
        if 'typical_p' in sched:
            typical_p = None
        trunc, force_rows = self._trunc_args(B, min_p, typical_p)
        rows = self._per_image(B, temperature, top_k, top_p, guidance_scale if guided else None, force=force_rows)
        top_k_list, top_p_list = (None, None) if rows is not None else self._filter_lists(top_k, top_p)
        if guided:
            if uncond is not None and (uncond.shape[0] != self._cond_rows(B) or uncond.numel() != self._cond_rows(B) * self.block_size_cond):
                raise ValueError(f'uncond of shape {tuple(uncond.shape)}; expected {(self._cond_rows(B), self.block_size_cond)} (the shape of cond)')
            if rows is None and not math.isfinite(float(guidance_scale)):
                raise ValueError(f'guidance_scale {guidance_scale} is not finite')
        eng = self._sampling_eng(amp)
        cbs = self._checked_codebooks(model_aux)
        xs = partial_sample.to(torch.long).contiguous()
        c = self._cond(cond, B, device)
        u = self._cond(uncond, B, device) if guided else None
        comp = self._compose_args(B, device) if guided else None
        keep, active = (None, None) if keep_mask is None else self._keep_flags(keep_mask, xs, start_loc)
        seeded = rows is not None and rows['seeds'] is not None
        seed, offset = (0, 0) if seeded else self._draw_rng(device, H * W * D)
        if not cached:
            return self._sample_uncached_scheduled(eng, xs, c, u, cbs, start_loc, sched, rows, trunc, temperature, top_k_list, top_p_list,
                                                   guidance_scale if guided else None, seed, offset, keep, active, comp=comp)
        nb = B if sched_per_image else 1
        arrays = {name: t.expand(nb, H * W, D).reshape(-1) for name, t in sched.items()}
        tr = self._trunc_engine(trunc)
        keep8, pos_active, start = None, None, start_loc
        if keep is not None:
            keep8 = keep.to(torch.uint8).contiguous()
            pos_active = [bool(a) for a in active.any(dim=1).tolist()]
            start = (0, 0)                                                   # (the kept prefix is part of `keep`)

        def run():
            eng.arm_schedule(per_image=sched_per_image, **arrays)
            if tr:
                eng.arm_trunc(*tr)
            if comp is not None:
                eng.arm_compose(*self._compose_flat(comp))
            try:
                if rows is not None:
                    return eng.sample_rows(xs, keep8, pos_active, c, u, cbs, start, rows['T'], rows['tk'], rows['tp'], rows['gs'] if guided else None,
                                           rows['seeds'], seed, offset, self.use_graph, **want)
                if guided:
                    return eng.sample_guided(xs, keep8, pos_active, c, u, cbs, start, temperature, float(guidance_scale), top_k_list, top_p_list,
                                             seed, offset, self.use_graph, **want)
                if keep is not None:
                    return eng.sample_masked(xs, keep8, pos_active, c, cbs, temperature, top_k_list, top_p_list, seed, offset, self.use_graph, **want)
                return eng.sample(xs, c, cbs, start_loc, temperature, top_k_list, top_p_list, seed, offset, self.use_graph, **want)
            finally:
                eng.arm_trunc(None, None)            # (a call refused before it reached the library leaves nothing armed)
                eng.arm_schedule()
                eng.arm_compose()
        return self._with_log_probs(want, self._on_side_stream(device, run))

    def _sample_uncached_scheduled(self, eng, xs, cond, uncond, cbs, start_loc, sched, rows, trunc, temperature, top_k_list, top_p_list,
                                   guidance_scale, seed, offset, keep, active, comp=None):
        """``cached=False`` inside schedule(): _sample_uncached with the values of every step sliced out of the tables the engine fills
        for the cached call -- the schedule where it gives a parameter, else the call's own values, broadcast -- and drawn by
        sample_logits_rows (sample_logits_trunc where a min-p / typical value is on anywhere).  Equal to the cached call bit for bit."""
        (H, W, D) = self.block_size
        B, device = xs.shape[0], xs.device
        guided = guidance_scale is not None

        def full(name, fallback, dtype):
            """(B, H*W, D): the schedule, or the call's values -- 1 or B rows of 1 or D values -- broadcast over the positions"""
            if name in sched:
                return sched[name].expand(B, H * W, D).to(dtype)
            return torch.tensor(fallback, dtype=dtype)[:, None, :].expand(B, H * W, D)
        if rows is not None:
            T = full('temperature', [[t] for t in rows['T']], torch.float32)
            K = full('top_k', rows['tk'], torch.int32)
            P = full('top_p', rows['tp'], torch.float32)
            G = full('guidance_scale', [[g] for g in rows['gs']], torch.float32) if guided else None
        else:
            T = full('temperature', [[float(temperature)]], torch.float32)
            K = full('top_k', [top_k_list], torch.int32)
            P = full('top_p', [top_p_list], torch.float32)
            G = full('guidance_scale', [[float(guidance_scale)]], torch.float32) if guided else None
        mp_rows = [[0.0] * D] if trunc is None else trunc['mp'] if trunc['per_image'] else [trunc['mp']]
        ty_rows = [[-1.0] * D] if trunc is None else trunc['ty'] if trunc['per_image'] else [trunc['ty']]
        Mp, Ty = full('min_p', mp_rows, torch.float32), full('typical_p', ty_rows, torch.float32)
        any_trunc = bool((Mp > 0).any()) or bool((Ty >= 0).any())
        T, K, P, Mp, Ty = (t.contiguous().to(device) for t in (T, K, P, Mp, Ty))
        sd = rows['seeds'] if rows is not None else None
        seeds_dev = None if sd is None else torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in sd], dtype=torch.int64, device=device)
        start = max(int(start_loc[0]) * W + int(start_loc[1]), 0)
        if keep is not None:
            xs = torch.where(keep, xs, torch.zeros_like(xs))                # (see sample(): the host loops embed every code)
        xs2, c2 = xs.clone(), cond
        if comp is not None:
            xs2, c2 = self._compose_rows_cat(comp, xs, cond, uncond)
        elif guided:
            xs2 = torch.cat([xs, xs])
            if cond is not None or uncond is not None:
                zeros = torch.zeros((B, self.block_size_cond), dtype=torch.long, device=device)
                c2 = torch.cat([zeros if cond is None else cond, zeros if uncond is None else uncond])
        for pos in range(start, H * W):
            h, w = divmod(pos, W)
            for d in range(D):
                if active is not None and not active[pos, d]:
                    continue                             # keep_mask: the code is given in every row
                logits = self._on_side_stream(device, lambda: eng.logits(xs2, c2, cbs))[:, h, w, d].contiguous()
                if self.vocab_size[d] < logits.shape[-1]:
                    logits[:, self.vocab_size[d]:] = float('-inf')          # LogitMask, as the sampling path applies it
                logits = self._anchor_step(logits, xs2, B, pos, d, guided)
                if comp is not None:
                    logits = self._compose_rows(logits, B, comp, G[:, pos, d].tolist())
                elif guided:
                    logits = self._guide_rows(logits[:B], logits[B:], G[:, pos, d].tolist())
                step = dict(seed=seed, offset=offset + pos * D + d)
                tkd = (T[:, pos, d].contiguous(), K[:, pos, d].contiguous(), P[:, pos, d].contiguous())
                if any_trunc:
                    idx = _native.sample_logits_trunc(logits, row_temperature=tkd[0], row_top_k=tkd[1], row_top_p=tkd[2],
                                                      row_min_p=Mp[:, pos, d].contiguous(), row_typical_p=Ty[:, pos, d].contiguous(),
                                                      row_seeds=seeds_dev, **step)[0]
                else:
                    idx, _ = _native.sample_logits_rows(logits, *tkd, seeds=seeds_dev, **step)
                if keep is not None:
                    idx = torch.where(keep[:, h, w, d], xs2[:B, h, w, d], idx)
                xs2[:, h, w, d] = torch.cat([idx] * (xs2.shape[0] // B)) if guided else idx
        return xs2[:B].contiguous() if guided else xs2

    def _keep_flags(self, keep_mask, xs, start_loc):
        """keep_mask of sample() -> (keep (B,H,W,D) bool on the device of `xs`, active (H*W, D) bool on the host: some row draws that
        code).  One device-to-host transfer carries both the activity and the range check of the kept codes: the engine embeds them,
        and its gather kernels trap on a code outside the vocabulary.  Codes that are not kept are not looked at."""
        (B, H, W, D) = xs.shape
        if not torch.is_tensor(keep_mask):
            keep_mask = torch.as_tensor(keep_mask)
        if keep_mask.dtype.is_floating_point or keep_mask.dtype.is_complex:
            raise ValueError(f'keep_mask of dtype {keep_mask.dtype}; expected bool or an integer type (nonzero = kept)')
        shp = tuple(keep_mask.shape)
        if shp == (B, H, W, D):
            km = keep_mask
        elif shp == (B, H, W) and shp == (H, W, D):
            raise ValueError(f'keep_mask of shape {shp} is both (B, H, W) and (H, W, D) here; pass it as {(B, H, W, D)}')
        elif shp == (B, H, W):
            km = keep_mask[..., None]
        elif shp == (H, W, D):
            km = keep_mask[None]
        elif shp == (H, W):
            km = keep_mask[None, :, :, None]
        else:
            raise ValueError(f'keep_mask of shape {shp}; expected {(B, H, W, D)}, {(B, H, W)}, {(H, W, D)} or {(H, W)}')
        keep = (km.to(xs.device) != 0).expand(B, H, W, D).clone()
        start = min(max(int(start_loc[0]) * W + int(start_loc[1]), 0), H * W)
        keep.view(B, H * W, D)[:, :start] = True
        vmax = torch.tensor(self.vocab_size, dtype=torch.long, device=xs.device)
        bad = (keep & ((xs < 0) | (xs >= vmax))).any()
        host = torch.cat([(~keep.view(B, H * W, D).all(dim=0)).reshape(-1), bad.reshape(1)]).cpu()
        if bool(host[-1]):
            raise ValueError(f'keep_mask keeps a code outside 0 .. vocab_size - 1 (vocab_size = {self.vocab_size})')
        return keep, host[:-1].view(H * W, D)

    def _sample_uncached(self, eng, xs, cond, cbs, start_loc, temperature, top_k_list, top_p_list, seed, offset, keep=None, active=None,
                         guidance_scale=None, rows=None, trunc=None, comp=None):
        """``cached=False`` (transformers.py:352-356): nothing is carried from one step to the next -- every step recomputes the
        logits of the whole code map from the codes drawn so far (one teacher-forced pass of the engine per step, 256 per
        batch, as slow as the reference's own uncached loop) and samples position (h, w, d) from them with the draw the
        cached path would make at that step (same Philox key: seed, offset + step).  It exists, as in the reference, as the
        cross-check of the cache: the codes equal ``cached=True`` bit for bit (tests/test_gpu_parity.py).  (Both paths step the
        engine with B rows per launch -- the teacher-forced pass is the cached stepping over given codes, not one (B*H*W*D)-row
        pass -- so both pick the same kernels for a given B)
        ``guidance_scale`` (sample_guided): `xs` / `cond` hold 2B rows, images then their unconditional twins; each step draws B rows
        from guide_logits of the two halves -- Philox row b, as the engine's guided sampler -- and writes the code to both halves;
        `keep` has B rows and the first B rows are returned.
        ``rows`` (per-image parameters, _rows_on_device): the draw is sample_logits_rows with the tables of the rows -- and
        guidance_scale a list, one scale per image -- in place of the scalars; with seeds, key seeds[b] and counter pos * D + d.
        ``trunc`` (_trunc_args): min-p / typical sampling, the draw by sample_logits_trunc with the depth's values (or tables).
        ``comp`` (_compose_args; with guidance_scale): `xs` / `cond` hold (2 + K) B rows, the K blocks under the extra conditions behind the
        twins; each step draws from compose_logits of the blocks and writes the code to all of them."""
        from ... import _native
        (H, W, D) = self.block_size
        start = max(int(start_loc[0]) * W + int(start_loc[1]), 0)
        xs = xs.clone()
        n = xs.shape[0] // (2 + (comp['K'] if comp is not None else 0)) if guidance_scale is not None else xs.shape[0]
        if trunc is not None and rows is not None:
            mp_dev, ty_dev = self._trunc_on_device(trunc, n, D, xs.device)
        for pos in range(start, H * W):
            h, w = divmod(pos, W)
            for d in range(D):
                if active is not None and not active[pos, d]:
                    continue                             # keep_mask: the code is given in every row
                logits = self._on_side_stream(xs.device, lambda: eng.logits(xs, cond, cbs))[:, h, w, d].contiguous()
                if self.vocab_size[d] < logits.shape[-1]:
                    logits[:, self.vocab_size[d]:] = float('-inf')          # LogitMask, as the sampling path applies it
                logits = self._anchor_step(logits, xs, n, pos, d, guidance_scale is not None)
                if comp is not None:
                    logits = self._compose_rows(logits, n, comp, guidance_scale)
                elif guidance_scale is not None and rows is not None:
                    logits = self._guide_rows(logits[:n], logits[n:], guidance_scale)
                elif guidance_scale is not None:
                    logits = _native.guide_logits(logits[:n].contiguous(), logits[n:].contiguous(), guidance_scale)
                if trunc is not None and rows is not None:
                    idx = _native.sample_logits_trunc(logits, row_temperature=rows['T_dev'], row_top_k=rows['tk_dev'][d], row_top_p=rows['tp_dev'][d],
                                                      row_min_p=mp_dev[d], row_typical_p=ty_dev[d], row_seeds=rows['seeds_dev'], seed=seed,
                                                      offset=offset + pos * D + d)[0]
                elif trunc is not None:
                    idx = _native.sample_logits_trunc(logits, temperature=temperature, top_k=top_k_list[d], top_p=top_p_list[d],
                                                      min_p=trunc['mp'][d], typical_p=trunc['ty'][d], seed=seed, offset=offset + pos * D + d)[0]
                elif rows is not None:
                    idx, _ = _native.sample_logits_rows(logits, rows['T_dev'], rows['tk_dev'][d], rows['tp_dev'][d], seeds=rows['seeds_dev'],
                                                        seed=seed, offset=offset + pos * D + d)
                else:
                    idx, _ = _native.sample_logits(logits, temperature, top_k_list[d], top_p_list[d], seed=seed,
                                                   offset=offset + pos * D + d)
                if keep is not None:
                    idx = torch.where(keep[:, h, w, d], xs[:n, h, w, d], idx)
                xs[:, h, w, d] = idx if guidance_scale is None else torch.cat([idx] * (xs.shape[0] // n))
        return xs if guidance_scale is None else xs[:n].contiguous()

    def _sample_torch_multinomial(self, eng, xs, cond, cbs, start_loc, temperature, top_k_list, top_p_list, keep=None, active=None,
                                  guidance_scale=None, rows=None):
        """``self.sampler = 'torch'`` (or RQAMD_SAMPLER=torch): the loop of transformers.py:346-364 driven from the host, one engine
        step per (h, w, d), the draw by ``torch.multinomial(probs, num_samples=1)`` on the filtered probabilities -- the call
        sample_from_logits makes (rqvae/utils/utils.py:112), so the device generator is consumed exactly as the reference consumes
        it (one multinomial over a (B, V) tensor per step).  ~10x slower than the default on-device sampler (no graphs, one host
        round per step); meant for seed-for-seed comparisons, not for throughput.
        ``guidance_scale`` (sample_guided): 2B rows are stepped, images then their unconditional twins; the B draws of a step come
        from guide_logits of the two halves and are set in both; `keep` has B rows and the first B rows are returned.
        ``rows`` (per-image parameters, _rows_on_device): the probabilities come from sample_logits_rows, every row filtered with its
        own values (and guidance_scale is a list, one scale per image)."""
        from ... import _native
        (H, W, D) = self.block_size
        start = max(int(start_loc[0]) * W + int(start_loc[1]), 0)
        n = xs.shape[0] // 2 if guidance_scale is not None else xs.shape[0]
        eng.step_begin(xs, cond, cbs)
        n_pos = H * W
        if active is not None:                         # keep_mask: nothing runs after the last position that draws a code
            drawn = active.any(dim=1).nonzero()
            n_pos = int(drawn[-1]) + 1 if len(drawn) else 0
        first = 0
        if self._prefix_one_pass():                    # the given leading positions in one pass (rqamd_rqt_step_prefill), as the engine's own loop
            while first < n_pos and (first < start or (active is not None and not active[first].any())):
                first += 1
            if 1 <= first < n_pos:
                eng.step_prefill(first)
            else:
                first = 0
        for pos in range(first, n_pos):
            if pos < start or (active is not None and not active[pos].any()):
                eng.step_logits(pos, -1)               # given codes: body KV cache only
                continue
            h, w = divmod(pos, W)
            for d in range(D):
                logits = eng.step_logits(pos, d)
                if active is not None and not active[pos, d]:
                    continue                           # given in every row: no draw (the step fed the head stack's KV cache)
                if guidance_scale is not None and rows is not None:
                    logits = self._guide_rows(logits[:n], logits[n:], guidance_scale)
                elif guidance_scale is not None:
                    logits = _native.guide_logits(logits[:n].contiguous(), logits[n:].contiguous(), guidance_scale)
                if rows is not None:
                    _, probs = _native.sample_logits_rows(logits.contiguous(), rows['T_dev'], rows['tk_dev'][d], rows['tp_dev'][d],
                                                          want_probs=True, want_samples=False)
                else:
                    _, probs = _native.sample_logits(logits, temperature, top_k_list[d], top_p_list[d], want_probs=True, want_samples=False)
                try:
                    idx = torch.multinomial(probs, num_samples=1).squeeze(-1)
                except RuntimeError:
                    print(probs, logits, torch.sum(probs), torch.sum(probs < 0))
                    raise
                if keep is not None:
                    idx = torch.where(keep[:, h, w, d], xs[:n, h, w, d], idx)
                eng.step_set_code(pos, d, idx if guidance_scale is None else torch.cat([idx, idx]))
        out = eng.step_end()
        return out if guidance_scale is None else out[:n].contiguous()

    @staticmethod
    def _draw_rng(device, n_steps):
        """(seed, offset) of the device's default generator, advanced past this call: set_seed(seed + rank)
        in the drivers (main_sampling_fid.py:166-169) therefore makes sampling reproducible per rank."""
        if device.type == 'cuda':
            gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
        else:
            gen = torch.default_generator
        seed = gen.initial_seed()
        try:
            offset = gen.get_offset()
            gen.set_offset(offset + 4 * ((n_steps + 3) // 4))
        except (RuntimeError, AttributeError):
            offset = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) * 4     # CPU generator (emulator tests)
        return seed, offset

    @staticmethod
    def _soft_ce_rows(logits, targets):
        """soft_target_cross_entropy(logits, targets, reduction='none') (rqvae/optimizer/loss.py:68-84) over the flattened rows, on the
        GPU (rqamd_soft_ce): any leading shape, fp32 or fp64 logits (the kernel computes in fp32), views made contiguous."""
        if logits.requires_grad:
            raise NotImplementedError('soft-target cross entropy of logits that require grad: this package has no backward pass '
                                      '(detach the logits to evaluate the loss)')
        if logits.shape != targets.shape:
            raise ValueError(f'soft targets of shape {tuple(targets.shape)} for logits of shape {tuple(logits.shape)}')
        V = logits.shape[-1]
        x = logits.detach().reshape(-1, V).to(torch.float32).contiguous()
        t = targets.detach().reshape(-1, V).to(device=x.device, dtype=torch.float32).contiguous()
        return _native.soft_ce(x, t)

    def compute_loss(self, logits, targets, use_soft_target=False):
        """transformers.py:371-382; use_soft_target: soft_target_cross_entropy (rqvae/optimizer/loss.py:68-84) on the GPU, no backward."""
        if use_soft_target:
            return self._soft_ce_rows(logits, targets).mean()
        return F.cross_entropy(logits.reshape(-1, logits.shape[-1]), targets.reshape(-1))

    def compute_cond_loss(self, cond_logits, conds):
        """transformers.py:383-391: next-token cross entropy of the conditioning prefix, cond_logits (B, T-1, Vc) against conds[:, 1:]."""
        assert cond_logits.shape[1] == conds.shape[1] - 1
        return F.cross_entropy(cond_logits.reshape(-1, cond_logits.shape[-1]), conds[:, 1:].reshape(-1))

    @torch.no_grad()
    def compute_codebook_loss(self, logits, targets, use_soft_target=False):
        """transformers.py:393-410: the cross entropy of each depth (codebook) separately, (D,); use_soft_target as in compute_loss."""
        D = logits.shape[-2]
        if use_soft_target:
            return self._soft_ce_rows(logits, targets).reshape(-1, D).mean(dim=0)
        per_code = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), targets.reshape(-1), reduction='none')
        return per_code.reshape(-1, D).mean(dim=0)
