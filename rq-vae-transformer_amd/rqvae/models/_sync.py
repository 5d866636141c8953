"""Parameter -> engine synchronisation shared by RQVAE and RQTransformer.

The engines keep packed bf16 copies of the nn.Parameters.  A cheap signature (storage pointer and
in-place version counter of every tensor) decides when they must be pushed again: after
``load_state_dict``, ``.to(device)``, ``.half()/.float()`` or any in-place edit."""
import torch


def _walk(module, out):
    for p in module._parameters.values():
        if p is not None:
            out.append(p)
    for b in module._buffers.values():
        if b is not None:
            out.append(b)
    for c in module._modules.values():
        if c is not None:
            _walk(c, out)


def signature(*modules):
    """(storage pointer, version counter, device, dtype) of every parameter and buffer below `modules`, in module-tree order.
    A walk over the live module tree (so replaced Parameters / sub-modules are seen) without building state_dict's prefixed
    names: ~0.25 ms for the 398 tensors of the RQ-VAE against 2.5 ms through state_dict -- it runs on every decode_code call of
    the drivers' one-image-per-call loops."""
    ts = []
    for m in modules:
        _walk(m, ts)
    return tuple([(t.data_ptr(), t._version, t.device, t.dtype) for t in ts])


def push_all(module, engine, skip_prefixes=()):
    with torch.no_grad():
        for k, v in module.state_dict(keep_vars=True).items():
            if any(k.startswith(p) for p in skip_prefixes) or not v.is_floating_point():
                continue                                  # integer buffers (TupleEmbedding.offsets) are derived from the config
            engine.set_param(k, v)


class SideStream:
    """hipGraph capture is illegal on the legacy default stream, which is what torch hands out as the current stream unless
    the caller set one.  The engines therefore run on a stream of their own, ordered after the caller's current stream on
    entry and before it on exit; results are tagged for the caller's stream (record_stream) so that the caching allocator
    does not recycle them early."""

    def __init__(self):
        self._stream = None

    def run(self, device, fn):
        if device.type != 'cuda':
            return fn()
        cur = torch.cuda.current_stream(device)
        if self._stream is None or self._stream.device != device:
            self._stream = torch.cuda.Stream(device=device)
        side = self._stream
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            out = fn()
        cur.wait_stream(side)
        def tag(o):                                   # (tuples may nest and hold None: sample(return_log_probs=True))
            if isinstance(o, tuple):
                for t in o:
                    tag(t)
            elif o is not None:
                o.record_stream(cur)
        tag(out)
        return out
