"""CPU: ovis_split_gemm_tn_map_slices (host-side, no GPU) scores the in-map rows of the small-map weight gradient and is
ovis_split_gemm_tn_slices for every shape that form does not serve."""


def _f():
    from cvpr22_cross_modal_pseudo_labeling_amd import _lib

    lib = _lib.load()
    return lib.ovis_split_gemm_tn_map_slices, lib.ovis_split_gemm_tn_slices


def _end(maps, h, w, tiles_per_tap, s, slots=512):
    """k-steps until the last resident slot ends when the taps with the most in-map rows are dispatched first."""
    import heapq

    cnts = sorted(((h - abs(dy)) * (w - abs(dx)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)), reverse=True)
    free, end = [], 0
    for cnt in cnts:
        steps = -(-maps * cnt // 32)
        length = -(-steps // s)
        for _ in range(tiles_per_tap * s):
            t = length + (heapq.heappop(free) if len(free) >= slots else 0)
            heapq.heappush(free, t)
            end = max(end, t)
    return end


def test_res5_weight_gradient_slots_end_together():
    new, old = _f()
    for maps in (2048, 1024):                     # student and teacher RoI counts
        s = new(maps * 49, 512, 512, 3, 3, 7, 7)
        assert s == 7
        steps = -(-maps * 49 // 32)
        # two rounds of uniform slices walk 2 * ceil(steps / 7) k-steps per slot; in-map rows, longest first: 13 % fewer
        assert _end(maps, 7, 7, 16, s) <= 0.875 * 2 * -(-steps // 7)


def test_other_shapes_keep_the_row_count_score():
    new, old = _f()
    for m, n, ch, kh, kw, h, w in ((8400, 256, 256, 3, 3, 50, 84), (33400, 128, 128, 3, 3, 100, 167), (100352, 512, 1024, 1, 1, 7, 7),
                                   (50, 128, 128, 3, 3, 7, 7),     # large maps, 1x1, rows that are no whole maps
                                   (64 * 200, 128, 128, 1, 19, 1, 64), (64 * 200, 128, 128, 25, 1, 64, 1),
                                   (49 * 200, 128, 128, 7, 3, 7, 7)):   # more than 5 taps a side: more than 3 x 3 classes
        assert new(m, n, ch, kh, kw, h, w) == old(m, n, ch, kh * kw)
    for m, n, ch in ((49, 128, 128), (49 * 70, 256, 256), (64 * 5, 128, 128)):
        s = new(m, n, ch, 3, 3, 7 if m % 49 == 0 else 8, 7 if m % 49 == 0 else 8)
        assert 1 <= s <= 256 and (s == 1 or (m + 31) // 32 // s >= 8)
    assert new(0, 128, 128, 3, 3, 7, 7) == 1
