"""The designed masks of tests/rle_cases.py against the host encoder (nuhtc_amd/cocomask.py): every case has the property it is named
after, so that tests/test_hip_rle.py compares the device encoder with strings that exercise each rule of maskApi.c rleEncode /
rleToString / rleToBbox.  Also the host-side surface of the device route: the --rle-on flag of tools/infer_wsi.py and pack_records."""
import os
import sys

import numpy as np
import pytest

from nuhtc_amd import cocomask
import rle_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = RC.H, RC.W


def counts_of(name):
    return cocomask.string_to_counts(RC.expected()[name][0].decode('ascii'))


def test_frames_are_not_square_and_multiples_of_32():
    fr = RC.frames()
    assert set(fr) == {(64, 96), (128, 128)}
    assert fr[(128, 128)] == ['big_empty_16384', 'big_pixel_last_16383', 'big_checkerboard']
    assert sum(n.startswith('blob_') for n in fr[(64, 96)]) == 200


def test_round_trip_of_every_case():
    for name, m in RC.cases().items():
        r = cocomask.encode(m)
        assert r['size'] == list(m.shape)
        assert np.array_equal(cocomask.decode(r), m), name
        assert sum(counts_of(name)) == m.size and cocomask.area(r) == int(m.sum()), name


def test_counts_of_the_boundary_cases():
    assert counts_of('empty') == [H * W]
    assert counts_of('full') == [0, H * W]
    assert counts_of('pixel_first') == [0, 1, H * W - 1]                 # the leading zero run is empty
    assert counts_of('pixel_last') == [H * W - 1, 1]                     # no trailing zero count
    y, x = H // 2 + 3, W // 2 - 5
    assert counts_of('pixel_mid') == [x * H + y, 1, H * W - x * H - y - 1]          # column-major: p = x * H + y
    assert counts_of('bar_crossing') == [40 * H + H - 4, 8, H * W - 41 * H - 4]     # ONE run across the column boundary
    assert counts_of('bar_gap') == [40 * H + H - 5, 4, 1, 4, H * W - 41 * H - 4]
    assert counts_of('word_seam_pixels') == [31 * H + 10, 1, H, 1, 31 * H, 1, H, 1, H * W - 64 * H - 14]
    assert len(counts_of('word_seam_row')) == 2 * 36 + 1
    assert counts_of('bottom_row_to_last_column')[-1] == 9 and len(counts_of('bottom_row_to_last_column')) % 2 == 0
    assert counts_of('big_empty_16384') == [16384] and counts_of('big_pixel_last_16383') == [16383, 1]
    cols = np.flatnonzero(RC.cases()['wider_than_a_wave'].any(0))
    assert cols[-1] - cols[0] + 1 > 64


def test_character_boundaries_of_one_value():
    """1 / 2 / 3 / 4 characters: 15 | 16, 511 | 512, 16 383 | 16 384 (5 bits per character, the top one a sign bit)."""
    n_chars = {15: 1, 16: 2, 511: 2, 512: 3, 16383: 3, 16384: 4}
    for L, k in n_chars.items():
        assert len(cocomask.counts_to_string([L])) == k
    for L in RC.FIRST_RUNS:
        assert counts_of(f'first_run_{L}')[:2] == [L, 3]
        assert len(RC.expected()[f'first_run_{L}'][0]) == n_chars[L] + 1 + len(cocomask.counts_to_string([H * W - L - 3]))
    assert len(RC.expected()['big_empty_16384'][0]) == 4 and len(RC.expected()['big_pixel_last_16383'][0]) == 3 + 1


def test_delta_cases_hit_the_sign_aware_stop_rule():
    n_chars = {-16: 1, -17: 2, 15: 1, 16: 2}
    for d in RC.DELTAS:
        c = counts_of(f'delta_{d:+d}')
        assert c[:6] == [7, 40, 9, 40 + d, 11, 5] and c[3] - c[1] == d
        s = RC.expected()[f'delta_{d:+d}'][0].decode('ascii')
        head = cocomask.counts_to_string([7, 40, 9])
        assert s.startswith(head)
        fourth = s[len(head):len(head) + n_chars[d]]
        assert not (ord(fourth[-1]) - 48) & 0x20 and all((ord(ch) - 48) & 0x20 for ch in fourth[:-1])          # exactly n_chars[d] characters
        assert cocomask.string_to_counts(head + fourth)[3] == 40 + d


def test_bbox_spans_the_full_height_for_crossing_runs_only():
    """rleToBbox looks at the two ends of every 1-run only and gives the full height to a run that ends in a later column than it began
    in: with that rule it is the box of the set pixels for every case.  The crossing bar is the case that needs the rule: its run starts
    at row H - 4 and ends at row 3, and the ends alone would give rows 3 .. H - 4."""
    full_height = []
    for name, m in RC.cases().items():
        ys, xs = np.nonzero(m)
        true = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)] if len(ys) else [0, 0, 0, 0]
        assert RC.expected()[name][1] == true, name
        crosses = bool((m[-1, :-1] & m[0, 1:]).any())              # some 1-run goes from the bottom of a column into the top of the next
        assert (RC.expected()[name][1][3] == m.shape[0]) == crosses, name
        if crosses:
            full_height.append(name)
    assert 'bar_crossing' in full_height and 'bar_gap' not in full_height and not any(n.startswith('blob_') for n in full_height)
    assert RC.expected()['bar_crossing'][1] == [40, 0, 2, H] and RC.expected()['bar_gap'][1] == [40, 0, 2, H - 1]
    assert RC.expected()['empty'][1] == [0, 0, 0, 0] and RC.expected()['full'][1] == [0, 0, W, H]


def test_only_the_checkerboard_exceeds_the_run_capacity():
    """The condition that bounds what the device test may leave to the fallback."""
    over = [name for name, e in RC.expected().items() if e[2] > RC.RUN_CAP]
    assert over == ['big_checkerboard'] and RC.expected()['big_checkerboard'][2] == 64 * 64 + 1
    assert max(e[2] for name, e in RC.expected().items() if name != 'big_checkerboard') < RC.RUN_CAP // 4


def test_pack_layout():
    m = RC.cases()['word_seam_pixels']
    w = RC.pack([m])[0].reshape(H, W // 32)
    assert w[10, 0] == 1 << 31 and w[11, 1] == 1 and w[12, 1] == 1 << 31 and w[13, 2] == 1 and int((w != 0).sum()) == 4


# ----------------------------------------------------------------------------- the tool's flag
def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import infer_wsi
    return infer_wsi


def test_rle_on_flag():
    infer_wsi = _tool()
    base = ['src', 'cfg', 'ckpt']
    assert infer_wsi.parse_args(base).rle_on == 'host'
    assert infer_wsi.parse_args(base + ['--rle-on', 'gpu']).rle_on == 'gpu'
    assert infer_wsi.parse_args(base + ['--rle-on', 'host']).rle_on == 'host'
    with pytest.raises(SystemExit):
        infer_wsi.parse_args(base + ['--rle-on', 'tpu'])


def test_rle_on_gpu_without_a_gpu_is_an_error(tmp_path, monkeypatch):
    import torch
    infer_wsi = _tool()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    args = [str(tmp_path / 'none.npy'), 'cfg', 'ckpt', '--save_dir', str(tmp_path / 'out'), '--rle-on', 'gpu']
    for mode in ('coco', 'all'):
        with pytest.raises(SystemExit) as e:
            infer_wsi.main(args + ['--mode', mode])
        assert '--rle-on gpu: no GPU is visible' in str(e.value)
    assert not (tmp_path / 'out').exists()


# ----------------------------------------------------------------------------- pack_records
def _records(n=5):
    rng = np.random.default_rng(3)
    rec = dict(tile=[], box=[], score=[], label=[], mask=[], ring=[])
    for i in range(n):
        h, w = int(rng.integers(2, 9)), int(rng.integers(2, 40))
        x0, y0 = int(rng.integers(0, 500)), int(rng.integers(0, 500))
        m = rng.random((h, w)) < 0.6
        m[0, 0] = True
        rec['tile'].append(i // 2)
        rec['box'].append(np.array([x0, y0, x0 + w, y0 + h], np.float64))
        rec['score'].append(float(rng.random()))
        rec['label'].append(int(rng.integers(0, 5)))
        rec['mask'].append((m, x0, y0))
        ring = rng.integers(0, 600, (int(rng.integers(3, 9)), 2)).astype(np.int64)
        rec['ring'].append(np.concatenate([ring, ring[:1]]))
    return rec


def test_pack_records_with_a_list_of_bytes_is_unchanged_and_the_blob_form_equals_it():
    from nuhtc_amd import wsi
    rec = _records()
    keep = [0, 2, 3]
    strings = [b'abc', b'', b'0123456789', b'xy', b'Q' * 37]            # one per record
    parts = wsi.pack_records(rec, keep, tile_base=7, rles=[strings[i] for i in keep])
    head, verts, crops, bits, blob = (p.numpy() for p in parts)
    assert head.shape == (3, 9) and head.dtype == np.float64 and blob.dtype == np.uint8
    assert head[:, 8].tolist() == [3, 10, 2] and blob.tobytes() == b'abc0123456789xy'
    assert head[:, 7].tolist() == [7 + rec['tile'][i] for i in keep] and head[:, 6].tolist() == [len(rec['ring'][i]) for i in keep]
    assert np.array_equal(head[:, :4], np.stack([rec['box'][i] for i in keep])) and head[:, 4].tolist() == [rec['score'][i] for i in keep]
    assert np.array_equal(verts, np.concatenate([rec['ring'][i] for i in keep]).astype(np.int32))
    mb, ma, mbits, moff = wsi.pack_masks([rec['mask'][i] for i in keep])
    assert np.array_equal(crops, np.concatenate([mb, ma[:, None], moff[:, None]], 1)) and np.array_equal(bits.view(np.uint32), mbits)
    none = wsi.pack_records(rec, keep, tile_base=7)
    assert none[0].numpy()[:, 8].tolist() == [0, 0, 0] and none[4].numel() == 0
    # the device's form: one blob of ALL records' strings + lengths; `keep` is taken inside
    whole = (np.frombuffer(b''.join(strings), np.uint8), np.array([len(s) for s in strings], np.int64))
    for a, b in zip(parts, wsi.pack_records(rec, keep, tile_base=7, rles=whole)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.numpy(), b.numpy())
    every = wsi.pack_records(rec, None, rles=whole)
    assert every[4].numpy().tobytes() == b''.join(strings) and every[0].numpy()[:, 8].tolist() == [len(s) for s in strings]


def test_records_take_device_strings_and_fall_back_to_the_host_encoder():
    """wsi._rle_of_records on a hand-made export: strings inside the pool are taken as they are, a length of -1 and a string that ends
    past the pool are encoded by cocomask.encode from the record's crop, and are counted."""
    from nuhtc_amd import wsi
    names = ['pixel_mid', 'word_seam_row', 'wider_than_a_wave', 'bar_gap', 'blob_007', 'blob_011']
    masks = [RC.cases()[k] for k in names]
    want = [RC.expected()[k] for k in names]
    ln = np.array([len(w[0]) for w in want], np.int32)
    ln[1] = -1                                                   # the device gave up on this one
    off = (np.cumsum(np.maximum(ln, 0)) - np.maximum(ln, 0)).astype(np.int32)
    pool = int(off[5]) + 2                                       # the last string ends past the pool: not written
    data = np.full(pool, 0xAA, np.uint8)
    for i in (0, 2, 3, 4):
        data[off[i]:off[i] + ln[i]] = np.frombuffer(want[i][0], np.uint8)
    bbox = np.array([w[1] for w in want], np.int32)
    bbox[1] = 0
    crops = []
    for m in masks:
        ys, xs = np.nonzero(m)
        crops.append((m[ys.min():ys.max() + 1, xs.min():xs.max() + 1].astype(bool), int(xs.min()), int(ys.min())))
    cb, _, bits, woff = wsi.pack_masks(crops)
    sizes = (cb[:, 3] - cb[:, 1]).astype(np.int64) * ((cb[:, 2] - cb[:, 0] + 31) // 32)
    g = dict(rle_len=ln, rle_off=off, rle_bbox=bbox, rle_bytes=data, rle_pool=pool)
    order = np.array([4, 1, 0, 5, 3, 2])                         # records come in another order than the export's rows
    pick = lambda a: a[order]
    blob, lens, boxes, hosted = wsi._rle_of_records(g, order, pick(cb).astype(np.int64), np.concatenate([bits[woff[k]:woff[k] + sizes[k]] for k in order]),
                                                    pick(sizes), (H, W))
    assert hosted == 2 and lens.tolist() == [len(want[k][0]) for k in order] and boxes.tolist() == [want[k][1] for k in order]
    assert blob.tobytes() == b''.join(want[k][0] for k in order)
