"""
GPU: the capture-and-replay protocol both mean-teacher steps share (graph_replay.GraphReplay) on a toy pass -- a few element-wise fp32
operations on 8-element tensors, one stream, nothing forked inside a capture: results are deterministic and compared bit for bit.
"""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _probed_streams():
    """The side-stream probe (it may warn about the queues it finds) runs once, in front of the tests that count warnings."""
    from cutmix_semisup_seg_amd import ops
    ops.pooled_stream(DEV, 'teacher')


def _fresh(seed, n=8):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, generator=g, device=DEV), torch.randn(n, generator=g, device=DEV)


def _toy(a, b, scale=1.0):
    return a * 2.0 + b * scale, [torch.sin(a) - b, a * b]


def _same(got, ref):
    return torch.equal(got[0], ref[0]) and len(got[1]) == len(ref[1]) and all(torch.equal(p, q) for p, q in zip(got[1], ref[1]))


def test_two_eager_calls_one_capture_then_replays_per_signature():
    from cutmix_semisup_seg_amd.graph_replay import GraphReplay
    replay = GraphReplay('the toy passes', 'CMS_TOY_GRAPH')
    calls = []

    def run(a, b, scale):
        def fn(ts, capturing):
            calls.append(capturing)
            return _toy(ts[0], ts[1], scale)
        return replay.run([a, b], (scale,), fn, nets=(), device=DEV)

    held = None
    for i in range(6):
        a, b = _fresh(i)
        got = run(a, b, 1.0)
        assert _same(got, _toy(a, b, 1.0)), i
        if i == 3:
            held = (got[0], got[0].clone(), got[1][1], got[1][1].clone())
    assert calls == [False, False, True]                      # the host function: two eager iterations and one capture
    assert torch.equal(held[0], held[1]) and torch.equal(held[2], held[3])         # call 4's outputs after calls 5 and 6: clones
    assert len(replay) == 1 and all('graph' in v and not v.get('failed') for v in replay.values())
    # other extras, then another shape: each signature warms up and captures on its own
    for k, (n, scale) in enumerate([(8, 0.5), (5, 1.0)]):
        del calls[:]
        for i in range(4):
            a, b = _fresh(10 * k + i, n)
            assert _same(run(a, b, scale), _toy(a, b, scale)), (n, scale, i)
        assert calls == [False, False, True]
        assert len(replay) == 2 + k and sum(1 for v in replay.values() if 'graph' in v) == 2 + k
    a, b = _fresh(99)
    assert _same(run(a, b, 1.0), _toy(a, b, 1.0)) and calls == [False, False, True]     # the first graph is still there


def test_static_buffers_keep_aliases_and_none():
    from cutmix_semisup_seg_amd.graph_replay import GraphReplay
    replay = GraphReplay('the toy passes', 'CMS_TOY_GRAPH')
    seen = []

    def fn(ts, capturing):
        if capturing:
            seen.append((ts[0] is ts[1], ts[2] is None, len(ts)))
        return _toy(ts[0] + ts[1], ts[3])

    for i in range(5):
        a, b = _fresh(20 + i)
        if i == 2:
            caller = (a, b)
        assert _same(replay.run([a, a, None, b], (), fn, nets=(), device=DEV), _toy(a + a, b)), i
    assert seen == [(True, True, 4)]
    (ent,) = replay.values()
    assert ent['static'][0] is ent['static'][1] and ent['static'][2] is None
    assert ent['static'][0] is not caller[0] and ent['static'][3] is not caller[1]      # the graph reads its own buffers
    # [a, c, b] with c a clone is another signature: it does not replay the aliased graph
    a, b = _fresh(30)
    assert _same(replay.run([a, a.clone(), None, b], (), fn, nets=(), device=DEV), _toy(a + a, b)) and len(replay) == 2


def test_registered_generator_draws_anew_in_every_replay():
    from cutmix_semisup_seg_amd.graph_replay import GraphReplay
    if not hasattr(torch.cuda.CUDAGraph, 'register_generator_state'):
        pytest.skip('this torch cannot register a generator with a graph')
    replay = GraphReplay('the toy passes', 'CMS_TOY_GRAPH')
    gen = torch.Generator(device=DEV).manual_seed(3)

    def fn(ts, capturing):
        return ts[0] + torch.randn(8, device=DEV, generator=gen), []

    x = torch.zeros(8, device=DEV)
    draws = [replay.run([x], (), fn, nets=(), device=DEV, generator=gen)[0] for _ in range(5)]
    assert all('graph' in v for v in replay.values())
    assert not torch.equal(draws[3], draws[4])                # two consecutive replays


def test_failed_capture_marks_the_arenas_stale_before_the_eager_fallback():
    """An operand cached per weight version DURING an aborted capture was allocated but never written: the fallback must make it
    again (ADVICE: one step trained on garbage)."""
    from cutmix_semisup_seg_amd.arena import ensure_arena
    from cutmix_semisup_seg_amd.graph_replay import GraphReplay
    net = torch.nn.Linear(2, 2).to(DEV)
    arena = ensure_arena(net)                                 # net._cms_arena
    replay = GraphReplay('the toy passes', 'CMS_TOY_GRAPH')
    calls, made = [], []

    def make():
        made.append(torch.cuda.is_current_stream_capturing())
        return torch.full((8,), 3.0, device=DEV)

    def fn(ts, capturing):
        calls.append(capturing)
        pad = arena.cached('layer', 'pad', torch.float32, make)
        ce = ts[0] * pad
        if capturing:
            raise ValueError('the toy pass cannot be captured')        # host code between two launches
        return ce + 1.0, [ts[1] - pad]

    ref = lambda a, b: (a * 3.0 + 1.0, [b - 3.0])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        for i in range(3):
            a, b = _fresh(40 + i)
            assert _same(replay.run([a, b], (), fn, nets=(net,), device=DEV), ref(a, b)), i
        assert calls == [False, False, True, False]
        assert made == [False, True, False]                   # once per weight version: eager, inside the capture, and AFTER it
        for i in range(3):
            a, b = _fresh(50 + i)
            assert _same(replay.run([a, b], (), fn, nets=(net,), device=DEV), ref(a, b)), i
    assert calls == [False, False, True, False, False, False, False]      # no second attempt
    assert made == [False, True, False]
    (ent,) = replay.values()
    assert ent.get('failed') and 'graph' not in ent
    runtime = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert len(runtime) == 1 and 'the toy passes could not be captured' in str(runtime[0].message) \
        and 'ValueError' in str(runtime[0].message)
