"""
CPU: the signature that keys a hipGraph capture (graph_replay.signature) -- shapes, dtypes, which inputs are ONE tensor, the caller's
extras. Two calls may share a captured graph exactly when their signatures are equal.
"""
import torch

from cutmix_semisup_seg_amd.graph_replay import signature


def _inputs():
    a, b = torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 8, 8, dtype=torch.uint8)
    return [a, a, None, b]


EXTRA = (1.0, (8, 8), True, torch.bfloat16)


def test_equal_shapes_dtypes_and_alias_pattern_give_equal_keys():
    k0, k1 = signature(_inputs(), EXTRA), signature(_inputs(), EXTRA)       # other tensor objects, other values would do too
    assert k0 == k1 and hash(k0) == hash(k1)
    ones = _inputs()
    ones[0].fill_(1.0)
    assert signature(ones, EXTRA) == k0
    assert signature(_inputs()) == signature(_inputs(), ())


def test_every_part_of_the_signature_changes_the_key():
    k0 = signature(_inputs(), EXTRA)
    a, _, _, b = _inputs()
    wide = torch.zeros(2, 3, 8, 9)
    assert signature([wide, wide, None, b], EXTRA) != k0                    # a slot's shape
    half = a.bfloat16()
    assert signature([half, half, None, b], EXTRA) != k0                    # a slot's dtype
    assert signature([a, a, torch.zeros(1), b], EXTRA) != k0                # None -> tensor
    assert signature([a, a, None, None], EXTRA) != k0                       # tensor -> None
    assert signature([a, a.clone(), None, b], EXTRA) != k0                  # the alias pattern
    assert signature([a, a, None, b], EXTRA[:-1] + (torch.float32,)) != k0  # the extras
    assert signature([a, a, None, b], ()) != k0


def test_alias_pattern_is_by_object_not_by_value():
    a, b = torch.zeros(4), torch.ones(4)
    c = a.clone()
    assert signature([a, a, b]) != signature([a, c, b])
    assert signature([a, a, b]) == signature([b, b, a])                     # same shapes, same pattern
    assert signature([a, c, b]) == signature([c, a, b])
    assert signature([a, b, a]) != signature([a, a, b])                     # which slots alias matters, not only how many
