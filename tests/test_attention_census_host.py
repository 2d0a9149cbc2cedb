"""Host side of tests/test_attention_census_gpu.py: the expected visible sets against a loop over the header's words, the claims
the count check rests on, and the constant of the backward census against the staged reference it is defined by."""
import math

import torch

from test_attention_census_gpu import BWD_CASES, C_BWD, rows_specs, staged_worst_ratio, visible


def test_visible_matches_the_header_word_for_word():
    for L, mask in [(7, (0, -1, 0, -1, 0)), (7, (1, -1, 0, -1, 0)), (9, (2, 3, 5, -1, 0)), (9, (2, 3, 5, 8, 8)), (9, (2, 4, 2, 4, 6))]:
        mode, r0, c0, r1, c1 = mask
        vis = visible(L, mask)
        for q in range(L):
            for j in range(L):
                masked = (mode == 1 and j > q) or (mode == 2 and ((q == r0 and j < c0) or (q == r1 and j < c1)))
                assert bool(vis[q, j]) == (not masked)


def test_rows_specs_cover_the_tile_boundaries_and_never_mask_a_whole_row():
    for L in (130, 579, 1152):
        specs = rows_specs(L)
        assert (65, 65, 66, 66) in specs
        for r in (63, 64, 65, 127, 128):
            cs = {c for (r0, c, r1, _) in specs if r0 == r and r1 == -1}
            assert {0, L - 1, r, 63, 64, 65}.issubset(cs) and any(c != r for c in cs)
        assert any(s[0] == -1 and s[2] >= 0 for s in specs)
        for s in specs:
            visible(L, (2,) + s)  # asserts that every row keeps a key


def test_count_check_margins():
    """log2 n +- 3e-6 rounds back to n over 1..4096, and the margin 1/4 log2(1 + 1/n) stays above 8.8e-5 there."""
    n = torch.arange(1, 4097, dtype=torch.float64)
    for e in (-3e-6, 3e-6):
        assert torch.equal(torch.round(torch.exp2(torch.log2(n) + e)), n)
    assert float((0.25 * torch.log2(1 + 1 / n)).min()) >= 8.8e-5
    assert math.isclose(float(torch.log2(n[63])), 6.0)


def test_backward_census_constant_is_twice_the_staged_references_worst_ratio():
    worst = staged_worst_ratio()
    print(f'staged reference against plain fp64 over {len(BWD_CASES)} cases: worst error / (2^-8 T) = {worst:.4f}')
    assert abs(worst - 1.3145) < 1e-3 and abs(C_BWD - 2 * worst) < 2e-3
