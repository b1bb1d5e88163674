"""
CPU-only: csrc/cps_math.hpp -- the functions the kernel of csrc/cps.hip is made of -- driven on the host by a small program of its
own (tests/hostcheck_cps) over every pixel of the GPU test's cases, against the fp64 restatement (tests/_cps_refs.py):
labels and all four counts, no pixel left out. Then what a margin cannot hold: real ties on exactly representable values, NaN logits,
a threshold that is exactly reached; the sizes at which the walk takes another shape; the refusals; and the same stand-alone program
once more under the host's address and undefined-behaviour sanitizers.
"""
import numpy as np
import pytest

import _cps_refs as R
import _hostcheck

CASES = [(name, align) for name in R.GEOMETRIES for align in (True, False)]


@pytest.fixture(scope='module')
def host():
    exe = _hostcheck.build('hostcheck_cps')

    def run(logits, size, align, program=exe, **kw):
        return R.hostcheck_run(program, logits, size, align, **kw)
    return run


@pytest.mark.parametrize('name,align', CASES, ids=lambda v: str(v))
def test_header_on_the_host_vs_reference_every_pixel(host, name, align):
    for kind, with_um, tau in R.variants():
        inp, ref = R.case(name, align, kind), R.reference(name, align, kind, with_um, tau)
        assert ref['gap'] >= R.GAP and (tau == 0 or ref['conf_margin'] >= R.CONF)
        um = dict(um0=inp['um0'], um1=inp['um1']) if with_um else {}
        for as_ranges in ((False, True) if kind != 'rand' else (False,)):
            got = host(inp['logits'], inp['size'], align, tau=tau, **um, **R.mask_args(inp, as_ranges))
            R.same(got, ref)
    # one validity map given, the other not: a missing map is all valid
    inp = R.case(name, align, 'rand')
    R.same(host(inp['logits'], inp['size'], align, mask=inp['mask'], um1=inp['um1'], tau=R.TAU),
           R.cps_labels(*inp['logits'], inp['size'], align, inp['m'], None, inp['um1'], R.TAU))


@pytest.mark.parametrize('name,align', [('main', True), ('tab2c19', False), ('c21', True)], ids=lambda v: str(v))
def test_label_maps_at_an_odd_address_are_written_byte_by_byte(host, name, align):
    inp, ref = R.case(name, align, 'rand'), R.reference(name, align, 'rand', True, R.TAU)
    R.same(host(inp['logits'], inp['size'], align, mask=inp['mask'], um0=inp['um0'], um1=inp['um1'], tau=R.TAU, vec=False), ref)


def test_one_class_labels_are_zero_and_confidence_is_one(host):
    g = np.random.RandomState(3)
    lg = [g.standard_normal((2, 1, 3, 3)).astype(np.float32) * 3 for _ in range(4)]
    mask = (g.uniform(size=(2, 5, 7)) > 0.5).astype(np.float32)
    for tau in (0.0, R.TAU, 1.0):                    # a confidence of exactly 1 reaches a threshold of 1
        for align in (True, False):
            got = host(lg, (5, 7), align, mask=mask, tau=tau)
            assert not got['label_a'].any() and not got['label_b'].any()
            assert got['stats'].tolist() == [70, 70, 70, 70]


def test_exact_ties_keep_the_first_index(host):
    """A dyadic geometry: 8 x 32 -> 32 x 128 without aligned corners puts every sample at a multiple of 1/8 between its taps, and
    with integer logits in [-2, 2] every upsampled value is an exact fp32 number: ties are real and labels must be the FIRST argmax."""
    g = np.random.RandomState(5)
    lg = [g.randint(-2, 3, size=(2, 4, 8, 32)).astype(np.float32) for _ in range(4)]
    mask = (g.uniform(size=(2, 32, 128)) > 0.5).astype(np.float32)
    ref = R.cps_labels(*lg, (32, 128), False, mask >= 0.5)
    assert ref['gap'] == 0.0                                                  # there are ties
    u = R.T.upsample(lg[0], (32, 128), False)
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64))        # and the values are exact
    R.same(host(lg, (32, 128), False, mask=mask), ref)


def test_nan_logits_follow_the_argmax_order_and_fail_the_threshold(host):
    g = np.random.RandomState(7)
    lg = [g.standard_normal((1, 3, 4, 4)).astype(np.float32) * 3 for _ in range(4)]
    lg[0][0, 1] = np.nan                                       # network a, image 0: class 1 is NaN everywhere
    lg[3][0, 2, 0, 0] = np.nan                                 # network b, image 1: class 2 at one corner
    mask = np.zeros((1, 4, 4), dtype=np.float32)
    mask[0, :2] = 1.0
    for tau in (0.0, R.TAU):
        got = host(lg, (4, 4), True, mask=mask, tau=tau)
        want_a = np.where(mask[0] >= 0.5, lg[1][0].argmax(0), 1)       # NaN counts as maximal
        want_b = np.where(mask[0] >= 0.5, np.where(np.isnan(lg[3][0]).any(0), 2, np.nan_to_num(lg[3][0], nan=-np.inf).argmax(0)),
                          lg[2][0].argmax(0))
        if tau == 0.0:
            assert np.array_equal(got['label_a'][0], want_a) and np.array_equal(got['label_b'][0], want_b)
            assert got['stats'].tolist() == [16, 16, 16, int((want_a == want_b).sum())]
        else:
            # a NaN confidence fails `>=`: those pixels are 255, and the prediction still counts for the agreement
            assert (got['label_a'][0][mask[0] < 0.5] == 255).all() and got['label_b'][0, 0, 0] == 255
            assert got['stats'][0] == 16 and got['stats'][3] == int((want_a == want_b).sum())
            ref = R.cps_labels(*lg, (4, 4), True, mask >= 0.5, tau=tau)
            R.same(got, ref)


@pytest.mark.parametrize('c,tau', [(2, 0.5), (4, 0.25)])
def test_a_threshold_exactly_reached_keeps_the_label(host, c, tau):
    """uniform logits: every probability is exactly 1 / C = tau, and `>=` keeps the label (`>=`, not `>`)"""
    lg = [np.full((1, c, 2, 3), 1.5, dtype=np.float32) for _ in range(4)]
    mask = np.zeros((1, 5, 6), dtype=np.float32)
    got = host(lg, (5, 6), True, mask=mask, tau=tau)
    assert not got['label_a'].any() and not got['label_b'].any() and got['stats'].tolist() == [30] * 4
    above = host(lg, (5, 6), True, mask=mask, tau=float(np.nextafter(np.float32(tau), np.float32(1))))
    assert (above['label_a'] == 255).all() and above['stats'].tolist() == [30, 0, 0, 30]


def test_all_invalid_gives_all_255_and_zero_counts(host):
    inp = R.case('main', True, 'rand')
    zero = np.zeros_like(inp['um0'])
    got = host(inp['logits'], inp['size'], True, mask=inp['mask'], um0=zero, um1=zero)
    assert (got['label_a'] == 255).all() and (got['label_b'] == 255).all() and got['stats'].tolist() == [0, 0, 0, 0]


# output sizes at which the walk takes another shape: fewer than four pixels per sample (no group of four), sample starts at every
# residue of four, one short of / exactly / one past a workgroup's 1024 pixels, an odd number of pixels in several samples
EDGES = [(1, 1, 1), (3, 1, 1), (5, 1, 3), (4, 1, 2), (3, 3, 3), (2, 1, 1023), (2, 32, 32), (3, 25, 41), (2, 5, 413)]


@pytest.mark.parametrize('n,H,W', EDGES, ids=lambda v: str(v))
def test_walk_edges(host, n, H, W):
    """No seed search here: tau = 0 and a top-two gap that leaves no doubt (logits on a coarse grid plus a per-class offset)."""
    for seed, (c, align) in enumerate(((5, True), (3, False))):
        g = np.random.RandomState(100 * seed + n + H + W)
        lg = [(g.randint(-8, 9, size=(n, c, 1, 1)) * 8 + np.arange(c).reshape(1, c, 1, 1)).astype(np.float32) for _ in range(4)]
        mask = (g.uniform(size=(n, H, W)) > 0.5).astype(np.float32)
        um0 = (g.uniform(size=(n, H, W)) > 0.3).astype(np.float32) if seed else None
        ref = R.cps_labels(*lg, (H, W), align, mask >= 0.5, um0, None)
        assert ref['gap'] >= 1.0
        for vec in (True, False):
            R.same(host(lg, (H, W), align, mask=mask, um0=um0, vec=vec), ref)


def test_host_driver_refuses_what_the_library_refuses(host):
    inp = R.case('one', True, 'rand')
    for over in (dict(n=0), dict(c=0), dict(c=65), dict(h=0), dict(w=-1), dict(H=0), dict(W=0), dict(n=65536), dict(h=10), dict(w=71),
                 dict(H=2 ** 16, W=2 ** 15)):
        host(inp['logits'], inp['size'], True, mask=inp['mask'], expect_code=2, **over)


def test_stand_alone_under_the_host_sanitizers(host):
    """The same program with its own main, built with -fsanitize=address,undefined, as a process of its own."""
    exe = _hostcheck.build('hostcheck_cps', sanitize=True)
    for name, align, kind in (('main', False, 'rand'), ('main', True, 'box'), ('c64', True, 'xbox'), ('ident', True, 'rand'),
                              ('one', False, 'box'), ('tab2c19', True, 'rand'), ('c21', False, 'rand')):
        inp, ref = R.case(name, align, kind), R.reference(name, align, kind, True, R.TAU)
        for vec in (True, False):
            R.same(host(inp['logits'], inp['size'], align, program=exe, um0=inp['um0'], um1=inp['um1'], tau=R.TAU, vec=vec,
                        **R.mask_args(inp, kind != 'rand')), ref)
    g = np.random.RandomState(9)
    for n, H, W in ((5, 1, 3), (3, 1, 1), (2, 1, 1025)):                       # heads and tails of the groups of four
        lg = [g.standard_normal((n, 4, 1, 1)).astype(np.float32) for _ in range(4)]
        got = host(lg, (H, W), True, program=exe, mask=np.ones((n, H, W), dtype=np.float32))
        assert got['label_a'].max() < 4 and got['stats'][0] == n * H * W
