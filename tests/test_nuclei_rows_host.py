"""Host test of the per-nucleus rows on their way from the records to the files (nuhtc_amd.nuclei, nuhtc_amd.wsi): every kind at once
through pack_records, a gather and gathered_rows.  No GPU."""
import numpy as np

from nuhtc_amd import nuclei, wsi


def _records(rank, n, kinds):
    """n records of one rank; row i of kind number k (its place in nuclei.KINDS) is filled with 1000 rank + 10 i + k."""
    sq = np.ones((4, 4), bool)
    rec = dict(tile=[], box=[], score=[], label=[], mask=[], ring=[])
    for i in range(n):
        x = y = 20 * i
        rec['tile'].append(i); rec['box'].append(np.array([x, y, x + 4, y + 4], np.float64)); rec['score'].append(0.9 - 0.1 * i); rec['label'].append(i % 3)
        rec['mask'].append((sq, x, y)); rec['ring'].append(np.array([[x, y], [x + 3, y], [x + 3, y + 3], [x, y + 3], [x, y]], np.int64))
        for kind in kinds:
            rec.setdefault(kind.key, []).append(np.full(kind.width, 1000 * rank + 10 * i + nuclei.KINDS.index(kind), kind.dtype))
    return rec


def _value(kind, rank, i):
    return 1000 * rank + 10 * i + nuclei.KINDS.index(kind)


def _check(kinds):
    # rank 0: three records, of which `keep` drops record 1; rank 1: two records, all kept
    gathered = [wsi.pack_records(_records(0, 3, kinds), [0, 2]), wsi.pack_records(_records(1, 2, kinds))]     # a list of lists: the "gather"
    sent = [(0, 0), (0, 2), (1, 0), (1, 1)]                                                                     # (rank, record), rank-major
    assert all(len(g) == 5 + len(kinds) for g in gathered)
    for at, kind in enumerate(kinds, 5):                                   # the parts behind the five document parts, in the order of the kinds
        for g, n in zip(gathered, (2, 3 - 1)):
            assert tuple(g[at].shape) == (n, kind.width) and g[at].numpy().dtype == kind.dtype, kind.key
        every = wsi.gathered_rows(kind, gathered, part=at)
        assert every.dtype == kind.dtype and every.shape == (4, kind.width)
        assert every[:, 0].tolist() == [_value(kind, r, i) for r, i in sent] and (every == every[:, :1]).all(), kind.key
        kept = [3, 0, 1]
        rows = wsi.gathered_rows(kind, gathered, kept, part=at)
        assert rows[:, 0].tolist() == [_value(kind, *sent[j]) for j in kept] and (rows == rows[:, :1]).all(), kind.key


def test_rows_of_every_kind_follow_their_records_through_pack_and_gather():
    assert [k.key for k in nuclei.KINDS] == ['feat', 'morph', 'tex']      # the order of the blob fields, the launches and the parts
    _check(nuclei.KINDS)
    gathered = [wsi.pack_records(_records(0, 3, nuclei.KINDS), [0, 2])]
    assert np.array_equal(wsi.gathered_features(gathered), wsi.gathered_rows(nuclei.FEAT, gathered, part=5))


def test_rows_of_the_texture_alone_sit_at_part_5():
    _check((nuclei.TEX,))
    part = wsi.pack_records(_records(0, 3, (nuclei.TEX,)), [0, 2])[5]
    assert tuple(part.shape) == (2, nuclei.TEX.width) and part[:, 0].tolist() == [_value(nuclei.TEX, 0, 0), _value(nuclei.TEX, 0, 2)]
