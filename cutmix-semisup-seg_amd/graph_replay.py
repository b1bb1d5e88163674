"""
Gradient passes as ONE hipGraph launch: the capture-and-replay protocol shared by the CutMix step (step.py, its separate passes) and the
VAT step (vat.py). The layer engines of the U-Nets issue thousands of launches per iteration through Python autograd and the GPU waits
for the host; after a few eager iterations of a signature the passes are captured once into a torch.cuda.CUDAGraph over static input
buffers and replayed. The rules, for every caller:

  * a signature is the shapes / dtypes / devices of the inputs, which of them are ONE tensor, and whatever else the caller's passes
    branch on (modes, ramp, ...): each signature warms up, captures and replays on its own;
  * the eager warm-up iterations settle everything lazy (initialisation, BatchNorm modes); what synchronises must have happened BEFORE the
    capture -- the side-stream probe above all;
  * operands derived from the weights (padded / transposed copies, frozen BatchNorm affines) are cached per weight version by the eager
    path: the capture must contain their refresh, so the arenas are marked stale first -- and again when a capture fails, because
    what the aborted capture cached was allocated but never written;
  * an operation the capture cannot hold raises inside it: warning, the signature keeps running launch by launch;
  * what a replay returns are clones: the graph's own outputs are overwritten by the next replay.
"""
import warnings

import torch

from . import ops


def signature(tensors, extra=()):
    """Key of a call: per slot of the flat list `tensors` (tensors and Nones) its (shape, dtype, device index) or None, the alias pattern
    (per slot the first slot holding the same tensor OBJECT, -1 for None) and the caller's extra hashables."""
    first = {}
    return (tuple(None if t is None else (tuple(t.shape), t.dtype, t.device.index) for t in tensors),
            tuple(-1 if t is None else first.setdefault(id(t), j) for j, t in enumerate(tensors)),
            tuple(extra))


def _touch_arenas(nets):
    for net in nets:
        a = getattr(net, '_cms_arena', None)
        if a is not None:
            a.touch()


class GraphReplay(dict):
    """The per-signature store {signature: {'seen', 'failed', 'graph', 'static', 'out'}} and the protocol on it. `what` names the passes
    and `env` the environment variable that switches the replay off, for the warning and the error of a failed capture."""

    def __init__(self, what, env):
        super(GraphReplay, self).__init__()
        self.what, self.env = what, env

    def run(self, tensors, extra, fn, nets, device, generator=None, warmup=2):
        """`fn(tensors, capturing=False)` launch by launch for the first `warmup` calls of a signature (and for ever after a failed
        capture), then `fn(static tensors, capturing=True)` captured once and replayed. `fn` -> (ce scalars, [consistency scalars]).
        `nets`: the networks whose weight arenas (`_cms_arena`) the passes read; `generator`: a CUDA generator the passes draw from
        (registered with the graph). The layer engines' side streams do not fork / join inside the capture."""
        key = signature(tensors, extra)
        alias = key[1]
        ent = self.setdefault(key, {'seen': 0})
        if 'graph' not in ent:
            ent['seen'] += 1
            if ent['seen'] <= warmup or ent.get('failed'):
                return fn(tensors, capturing=False)
            static = []
            for j, t in enumerate(tensors):             # aliases and None preserved: each distinct tensor is cloned once
                static.append(None if t is None else (static[alias[j]] if alias[j] != j else t.clone()))
            _touch_arenas(nets)
            # (a trainer whose eager iterations never asked for a pooled stream met the probe inside the capture: `operation not
            # permitted when stream is capturing`)
            ops.pooled_stream(device, 'teacher')
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            if generator is not None and hasattr(g, 'register_generator_state'):
                g.register_generator_state(generator)
            prev = ops.set_side_streams_enabled(False)
            try:
                with torch.cuda.graph(g):
                    out = fn(static, capturing=True)
            except Exception as e:               # noqa: BLE001 -- an operation the capture cannot hold (nothing ran on the device)
                warnings.warn('cutmix-semisup-seg_amd: {} could not be captured into a hipGraph ({}: {}); this signature keeps running '
                              'launch by launch'.format(self.what, type(e).__name__, str(e).splitlines()[0] if str(e) else ''),
                              RuntimeWarning, stacklevel=3)
                ent['failed'] = True
                try:
                    torch.cuda.synchronize()
                except Exception as e2:          # noqa: BLE001 -- a forked stream is still inside the aborted capture: this process cannot launch any more
                    raise RuntimeError('a failed hipGraph capture left the device in capture mode ({}); restart with {}=0 (launch by launch) '
                                       'and report the operation named in the warning above'.format(e2, self.env)) from e
            finally:
                ops.set_side_streams_enabled(prev)
            if ent.get('failed'):
                _touch_arenas(nets)              # what the aborted capture cached per weight version was never written
                return fn(tensors, capturing=False)
            ent.update(graph=g, static=static, out=out)
        for j, (st, t) in enumerate(zip(ent['static'], tensors)):
            if t is not None and alias[j] == j:
                st.copy_(t)
        ent['graph'].replay()
        ce_sc, cons_vals = ent['out']
        return ce_sc.clone(), [c.clone() for c in cons_vals]
