"""Row maps of the row-compact reference pass (LlavaHipEngine.forward_hidden(prefix_dedup=True)).

A DPO batch is concatenated as [chosen 0..B-1 ; rejected 0..B-1].  The two sequences of pair i are `prompt + chosen` and
`prompt + rejected` padded on the right, so their MERGED sequences (text tokens and image feature slots) agree on a prefix of P_i
positions: same source, same attention mask, same position id.  Attention is causal and every other operator of a decoder layer works
row by row, so in every layer the rejected sequence's first P_i rows repeat the chosen sequence's.  A no-grad pass keeps one copy:

    compact_rows [M']   the kept dense rows (b * S + s), ascending: every chosen row, then the rows s >= P_i of every rejected sequence
    dense_src    [M]    for every dense row the compact row that holds its value (a dropped row names its chosen twin)

The policy's training pass (forward_hidden(save=True, prefix_dedup_rows=True)) keeps one copy too and needs two more maps for its
backward (build_policy_plan): dense_own, through which a gradient on kept rows is expanded with zeros on the dropped ones, and twin,
through which a dense gradient is folded - a shared row receives the sum of its two copies.

Pure tensor code: runs on CPU tensors (tests/test_prefix_dedup_host.py, tests/test_prefix_dedup_policy_host.py) and on the device
tensors of the engine alike."""
from typing import Sequence, Tuple

import torch


def source_key(src: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """What every merged position is built from, comparable across batch rows: src [Bn, S] is the merge map of vlr_merge_index
    (>= 0: index of a text token in its own row of ids [Bn, T]; < 0: an image feature slot of the deduplicated feature table, or
    the all-zero row).  -> int64 [Bn, S]: the token ID of a text slot (>= 0), the slot code itself otherwise (< 0)."""
    s = src.long()
    tok = torch.gather(ids.long(), 1, s.clamp(min=0))
    return torch.where(s >= 0, tok, s)


def shared_prefix_lengths(key: torch.Tensor, mask: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """P_i of the B pairs of a [chosen ; rejected] batch ([2B, S] each): the longest common prefix of the two merged sequences with
    equal source key, mask and position.  0 <= P_i <= S (P_i = S: the pair's sequences are identical).  -> int64 [B]"""
    if key.dim() != 2 or key.shape[0] % 2 or key.shape != mask.shape or key.shape != pos.shape:
        raise ValueError(f"shared_prefix_lengths: [2B, S] tensors expected, got {tuple(key.shape)}, {tuple(mask.shape)}, {tuple(pos.shape)}")
    B = key.shape[0] // 2
    eq = (key[:B] == key[B:]) & (mask[:B] == mask[B:]) & (pos[:B] == pos[B:])
    return eq.long().cumprod(dim=1).sum(dim=1)


def build_row_maps(P: Sequence[int], S: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(compact_rows int32 [M - sum P], dense_src int32 [M]) of B = len(P) pairs of S merged positions, M = 2 B S; CPU tensors.
    Invariants: compact_rows is strictly ascending and holds every chosen row; dense_src[compact_rows[j]] == j; the dropped row
    (B + i) * S + s, s < P_i, maps to the compact row of the chosen row i * S + s."""
    P = [int(p) for p in P]
    B = len(P)
    if B < 1 or S < 1 or any(p < 0 or p > S for p in P):
        raise ValueError(f"build_row_maps: prefix lengths {P} outside 0 .. S = {S}")
    s = torch.arange(S).unsqueeze(0)
    keep = torch.ones(2 * B, S, dtype=torch.bool)
    keep[B:] = s >= torch.tensor(P).unsqueeze(1)
    flat = keep.reshape(-1)
    compact_rows = torch.nonzero(flat).reshape(-1)
    index = torch.cumsum(flat.long(), 0) - 1                   # compact index of a KEPT dense row
    twin = torch.arange(2 * B * S).reshape(2 * B, S)
    twin[B:] = torch.where(keep[B:], twin[B:], twin[:B])       # a dropped rejected row reads its chosen twin
    dense_src = index[twin.reshape(-1)]
    return compact_rows.int(), dense_src.int()


def build_twin(compact_rows: torch.Tensor, dense_src: torch.Tensor) -> torch.Tensor:
    """twin int32 [Mc] of a pair of row maps: the dense index of the dropped row that reads kept row j (dense_src names j and the row is
    not kept), -1 for a kept row that stands for itself alone.  A kept row has at most one dropped copy (the rejected sequence's)."""
    M, Mc = int(dense_src.numel()), int(compact_rows.numel())
    kept = torch.zeros(M, dtype=torch.bool)
    kept[compact_rows.long()] = True
    dropped = torch.nonzero(~kept).reshape(-1)
    twin = torch.full((Mc,), -1, dtype=torch.int64)
    twin[dense_src.long()[dropped]] = dropped
    return twin.int()


def build_policy_plan(P: Sequence[int], S: int) -> dict:
    """Row maps of the row-compact POLICY pass (forward and backward) of B = len(P) pairs of S merged positions; CPU tensors.
    The last pair's prefix is lowered by up to 7 rows (never below 0; what it lacks is taken from the pair before it) so that
    Mc % 8 == 0: the kept rows are then merely computed twice, which is always valid, and the joint weight-gradient launch, which
    contracts over the Mc rows, keeps its 16-byte K alignment.  (With fewer shared rows than the trim in the whole batch Mc = M stays
    as it is; the caller - who checks plan["Mc"] % 8 and plan["shared"] - runs dense then.)
        P, shared, M, Mc, tail     the trimmed prefixes, their sum, the dense and compact row counts, S - P[-1]
        compact_rows [Mc], dense_src [M]    build_row_maps of the trimmed prefixes
        dense_own [M]   the compact row of a kept dense row, -1 for a dropped row (vlr_expand_rows_zero)
        twin [Mc]       the dense index of the dropped twin of a shared compact row, -1 otherwise (vlr_fold_rows)"""
    P = [int(p) for p in P]
    B = len(P)
    if B < 1 or S < 1 or any(p < 0 or p > S for p in P):
        raise ValueError(f"build_policy_plan: prefix lengths {P} outside 0 .. S = {S}")
    M = 2 * B * S
    trim = (-(M - sum(P))) % 8                                 # rows to keep again: (Mc + trim) % 8 == 0
    for i in range(B - 1, -1, -1):                             # the last pair's; a last prefix shorter than the trim leaves the rest to the pair before it
        take = min(trim, P[i])
        P[i] -= take
        trim -= take
    compact_rows, dense_src = build_row_maps(P, S)
    Mc = int(compact_rows.numel())
    own = torch.full((M,), -1, dtype=torch.int64)
    own[compact_rows.long()] = torch.arange(Mc)
    dropped = torch.nonzero(own < 0).reshape(-1)               # dense rows (B + i) * S + s, s < P_i
    twin = torch.full((Mc,), -1, dtype=torch.int64)
    twin[dense_src.long()[dropped]] = dropped
    return dict(P=P, shared=sum(P), M=M, Mc=Mc, tail=S - P[-1], compact_rows=compact_rows, dense_src=dense_src,
                dense_own=own.int(), twin=twin.int())
