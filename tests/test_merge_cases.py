"""tests/merge_cases.py reaches what it claims (oracle and numpy only): the branches of csrc/merge.hip that the designed
shapes and offsets are there for, and the size of the threshold sweep that tests/test_hip_merge.py runs over them."""
import numpy as np
import pytest

import merge_cases as MC

MODES = ('polygon', 'mask')


def test_shapes_have_the_layout_their_names_promise():
    s = MC.shapes()
    assert [s[f'frag{r}'].shape[1] for r in (16, 24, 40)] == [33, 49, 81]                   # 2, 2 and 3 words per row
    for c in MC.PINCH_COLS:
        left, right = s[f'pinch{c - 1}|{c}'], s[f'pinch{c - 1}|{c}_mirror']                  # the larger part left / right of the touch point
        for m in (left, right):
            assert not (m[11] & m[12]).any() and not m[11, c - 1:c + 1].all() and not m[12, c - 1:c + 1].all()       # no shared side
        assert left[11, c - 1] and left[12, c] and right[11, c] and right[12, c - 1]         # one diagonal step across the boundary
        assert left[:12, :c].sum() > left[12:, c:].sum() > 0 == left[:12, c:].sum() + left[12:, :c].sum()
        assert right[:12, c:].sum() > right[12:, :c].sum() > 0 == right[:12, :c].sum() + right[12:, c:].sum()
    b = s['bridge_over_32']
    assert b[5, 28:37].all() and b[4, 28:37].sum() == 0 == b[6, 28:37].sum()                # one pixel high, crosses column 32
    assert b[:, :28].sum() != b[:, 37:].sum()                                                # lobes of unequal size: no tie between the parts
    sp = s['spur_to_64']
    assert sp.shape[1] == 65 and sp[4, 64] and sp[:, 64].sum() == 1 and sp[:, 57:].sum() == 8
    r = s['ring_island_at_32']
    assert r.shape == (48, 100) and r[14, 32] and not r[14, 8:32].any() and not r[8:14, 8:92].any() and not r[20:28, 40:64].any()
    for name, col in (('second_comp_at_32', 32), ('second_comp_at_0', 0)):
        ys, xs = np.nonzero(s[name][8:])                                                     # the component found last
        assert not s[name][6:8].any() and xs.min() == col and (ys == 0).any()
    assert s['big150_hole'].shape == (150, 150) and not s['big150_hole'][50:90, 60:100].any()


@pytest.mark.parametrize('name', MC.PINCH + ('bridge_over_32',))
def test_pinched_rings_have_several_parts(name):
    from oracle.merge_poly import Poly
    ring = MC.rings()[name]
    assert Poly(ring, largest_part=False).area8 > Poly(ring).area8 > 0


@pytest.mark.parametrize('name', MC.SEVERAL_RINGS)
def test_island_and_fragment_cases_have_several_rings(name):
    from oracle.contour import find_contours_tree
    assert len(find_contours_tree(MC.shapes()[name])[0]) > 1


def test_only_the_selected_component_counts():
    """The two-component crops: the ring is that of the component found last, the other one adds nothing."""
    from oracle.merge_poly import Poly
    for name in ('second_comp_at_32', 'second_comp_at_0'):
        ring = MC.rings()[name]
        assert ring[:, 1].min() == 8 and Poly(ring).area8 == 8 * 5 * 7
    ring = MC.rings()['ring_island_at_32']
    assert ring[:, 0].min() == 2 and ring[:, 0].max() == 97                                  # the outer block, not the island


def test_placement_keeps_pairs_apart():
    masks, scores = MC.placed()
    assert len(masks) == 2 * len(MC.pairs()) == len(scores)
    b = np.array([[x, y, x + m.shape[1], y + m.shape[0]] for m, x, y in masks]).reshape(-1, 2, 4)
    lo, hi = b[:, :, :2].min(1), b[:, :, 2:].max(1)                                          # hull of each pair
    assert lo.min() >= 0
    k = np.arange(len(lo))
    cell = np.stack([k % MC.PER_ROW, k // MC.PER_ROW], 1) * MC.PITCH + MC.MARGIN
    assert (lo > cell - MC.MARGIN).all() and (hi < cell + MC.PITCH - MC.MARGIN).all()      # every pair inside its own pitch square
    assert len({MC.position(k)[0] % 64 for k in range(len(lo))}) == 64                       # positions relative to the grid cells vary
    assert ((hi - lo).max(1) > 3 * 64).any()


def test_every_pair_runs_in_both_score_orders():
    p = MC.pairs()
    assert {q[:4] for q in p if q[4]} == {q[:4] for q in p if not q[4]}
    offs = {q[2:4] for q in p if q[0] == q[1] == 'rect9x65'}
    assert offs == set(MC.OFFSETS)
    for a in MC.shapes():
        assert {q[1] for q in p if q[0] == a} == {a, *MC.CROSS_TARGETS}


@pytest.mark.parametrize('mode', MODES)
def test_reference_values_reach_the_branches(mode):
    inter, uni, r = MC.reference(mode)
    p = MC.pairs()
    assert all(0 <= i <= u for i, u in zip(inter, uni))
    wide = sum(1 for k, (a, b, dx, dy, _) in enumerate(p) if MC.inter_width(a, b, dx, dy) > 32 and inter[k] > 0)
    assert wide >= 20, wide
    assert int(((r > 0) & (r < 1)).sum()) >= 20
    zero = sum(1 for k, (a, b, dx, dy, _) in enumerate(p) if r[k] == 0.0 and MC.boxes_intersect(a, b, dx, dy))
    assert zero >= 5, zero
    assert (r == 1.0).any()
    distinct = len(set(r.tolist()))
    print(f'{mode}: {len(p)} pairs, {distinct} distinct values')
    assert distinct <= 300, distinct                                                         # bounds the GPU time of the sweep


def test_disjoint_offsets_are_disjoint():
    for name, offs in MC.DISJOINT.items():
        for dx, dy in offs:
            assert MC.boxes_intersect(name, name, dx, dy) and MC._mask_ref(name, name, dx, dy)[0] == 0, (name, dx, dy)


def test_polygon_reference_on_hand_worked_pairs():
    """A 9 x 33 rectangle's ring runs through the pixel centres: 8 x 32 cells.  Shifted by (5, 3): 5 x 27 cells shared."""
    assert MC._poly_ref('rect9x33', 'rect9x33', 5, 3) == (8 * 5 * 27, 8 * (2 * 8 * 32 - 5 * 27))
    assert MC._poly_ref('rect9x33', 'rect9x33', 32, 0) == (0, 8 * 2 * 8 * 32)                # one shared column of pixels: no area
    assert MC._poly_ref('rect1x40', 'rect1x40', 1, 0) == (0, 0)
    assert MC._mask_ref('rect9x33', 'rect9x33', 32, 0) == (9, 2 * 9 * 33 - 9)
    assert MC._mask_ref('rect9x33', 'rect9x33', -33, 0) == (0, 2 * 9 * 33)
    # the pinch keeps the 12-row part only: 11 x 13 cells, or 11 x 39
    assert MC._poly_ref('pinch32|33', 'pinch32|33', 0, 0) == (8 * 11 * 13,) * 2
    assert MC._poly_ref('pinch63|64', 'pinch63|64', 0, 0) == (8 * 11 * 39,) * 2
