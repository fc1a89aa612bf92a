"""The row maps of the row-compact reference pass (vlrlhf/prefix_dedup.py) on hand-made merged sequences: pure CPU tensors, no library.

A merged sequence is a list of sources: a token id (>= 0) or an image feature slot (< 0, the code vlr_merge_index writes: -(row + 1)).
Sequences are padded on the right with the all-zero row (source INT32_MIN, mask 0, position 1), as the merge of a right-padded batch is."""
import pytest
import torch

from vlrlhf import prefix_dedup as PD

ZERO = -(2 ** 31)


def merged(seqs):
    """[chosen 0..B-1 ; rejected 0..B-1] lists of sources -> (key, mask, pos) [2B, S]"""
    S = max(len(s) for s in seqs)
    key = torch.full((len(seqs), S), ZERO, dtype=torch.int64)
    mask = torch.zeros(len(seqs), S, dtype=torch.int32)
    for b, s in enumerate(seqs):
        key[b, :len(s)] = torch.tensor(s, dtype=torch.int64)
        mask[b, :len(s)] = 1
    pos = (mask.cumsum(1) - 1).int()
    pos[mask == 0] = 1
    return key, mask, pos


IMG = [-1, -2, -3, -4]                                   # one image of four feature slots
PROMPT = [1, 11, 12] + IMG + [13, 14]                    # the image inside the prompt


def check_maps(key, mask, pos, expect_P):
    Bn, S = key.shape
    B, M = Bn // 2, Bn * S
    P = PD.shared_prefix_lengths(key, mask, pos).tolist()
    assert P == list(expect_P), (P, expect_P)
    rows, dsrc = PD.build_row_maps(P, S)
    assert rows.dtype == torch.int32 and dsrc.dtype == torch.int32
    rows, dsrc = rows.long(), dsrc.long()
    assert rows.numel() == M - sum(P)                                                    # M' = M - sum P_i
    assert dsrc.numel() == M
    assert bool((rows[1:] > rows[:-1]).all())                                            # strictly ascending
    assert 0 <= int(rows.min()) and int(rows.max()) < M
    assert torch.equal(rows[:B * S], torch.arange(B * S))                                # every chosen row is kept
    assert torch.equal(dsrc[rows], torch.arange(rows.numel()))                           # dense_src[compact_rows[j]] == j
    assert 0 <= int(dsrc.min()) and int(dsrc.max()) < rows.numel()
    kept = torch.zeros(M, dtype=torch.bool)
    kept[rows] = True
    fk, fm, fp = key.reshape(-1), mask.reshape(-1), pos.reshape(-1)
    for m in torch.nonzero(~kept).reshape(-1).tolist():                                  # every dropped row ...
        b, s = divmod(m, S)
        twin = int(rows[dsrc[m]])
        assert b >= B and s < P[b - B]                                                   # ... is a rejected prompt row
        assert twin == (b - B) * S + s and kept[twin]                                    # ... mapped to a kept row of its pair, same position in the sequence
        assert fk[m] == fk[twin] and fm[m] == fm[twin] and fp[m] == fp[twin]             # ... with equal source, mask and position
    for i in range(B):                                                                   # the prefix is maximal
        if P[i] < S:
            c, r = i * S + P[i], (B + i) * S + P[i]
            assert fk[c] != fk[r] or fm[c] != fm[r] or fp[c] != fp[r]
    return rows, dsrc


def test_no_shared_prefix():
    key, mask, pos = merged([[1, 5, 6, 7], [2, 5, 6, 7]])
    rows, dsrc = check_maps(key, mask, pos, [0])
    assert torch.equal(rows, torch.arange(8)) and torch.equal(dsrc, torch.arange(8))     # the identity: nothing is dropped


def test_prefix_differs_per_pair_three_pairs():
    ch = [PROMPT + [20, 21, 22], [1, 30, 31, 32, 33], [1, 40, 41] + IMG + [42, 43, 44]]
    rj = [PROMPT + [25, 26], [1, 30, 35, 36, 37, 38], [9, 40, 41] + IMG + [42, 43, 44]]
    key, mask, pos = merged(ch + rj)
    check_maps(key, mask, pos, [len(PROMPT), 2, 0])


def test_identical_pair_drops_the_whole_rejected_sequence():
    seq = PROMPT + [20, 21]
    key, mask, pos = merged([seq, [1, 2, 3], seq, [1, 2, 4]])
    S = key.shape[1]
    rows, dsrc = check_maps(key, mask, pos, [S, 2])                                      # P = S, right padding included
    assert torch.equal(dsrc[2 * S:3 * S], torch.arange(S))                               # rejected 0 reads chosen 0 row for row


@pytest.mark.parametrize("chosen_len,rejected_len", [(6, 2), (2, 6)])
def test_ragged_right_padded_responses(chosen_len, rejected_len):
    ch = PROMPT + list(range(100, 100 + chosen_len))
    rj = PROMPT + list(range(200, 200 + rejected_len))
    key, mask, pos = merged([ch, rj])                                                    # B = 1
    check_maps(key, mask, pos, [len(PROMPT)])


def test_padding_after_equal_responses_still_matches():
    """a response that is a prefix of the other: the shared rows end where the shorter sequence's padding starts (mask differs)"""
    key, mask, pos = merged([PROMPT + [50, 51], PROMPT + [50, 51, 52, 53]])
    check_maps(key, mask, pos, [len(PROMPT) + 2])


def test_image_slot_straddles_the_prefix_end():
    ch = [1, 11] + IMG + [13]
    rj = [1, 11] + [-1, -2, -7, -8] + [13]                                               # another image from the third slot on
    key, mask, pos = merged([ch, rj])
    check_maps(key, mask, pos, [4])


def test_mask_or_position_difference_ends_the_prefix():
    key, mask, pos = merged([[1, 5, 6, 7], [1, 5, 6, 7]])
    mask2 = mask.clone()
    mask2[1, 2] = 0
    assert PD.shared_prefix_lengths(key, mask2, pos).tolist() == [2]
    pos2 = pos.clone()
    pos2[1, 1:] += 1
    assert PD.shared_prefix_lengths(key, mask, pos2).tolist() == [1]


def test_source_key_compares_token_ids_not_token_indices():
    ids = torch.tensor([[1, 7, 99, 8], [1, 7, 99, 9]])                                   # 99 = <image> (two slots)
    src = torch.tensor([[0, 1, -1, -2, 3, ZERO], [0, 1, -1, -2, 3, ZERO]], dtype=torch.int32)
    key = PD.source_key(src, ids)
    assert key.tolist() == [[1, 7, -1, -2, 8, ZERO], [1, 7, -1, -2, 9, ZERO]]
    mask = torch.tensor([[1, 1, 1, 1, 1, 0]] * 2)
    pos = torch.tensor([[0, 1, 2, 3, 4, 1]] * 2)
    assert PD.shared_prefix_lengths(key, mask, pos).tolist() == [4]


def test_bad_arguments():
    with pytest.raises(ValueError):
        PD.build_row_maps([5], 4)
    with pytest.raises(ValueError):
        PD.build_row_maps([-1], 4)
    with pytest.raises(ValueError):
        PD.shared_prefix_lengths(torch.zeros(3, 4), torch.zeros(3, 4), torch.zeros(3, 4))
