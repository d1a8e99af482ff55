"""The occlusion scan driver (transformercvn.hip.occlusion.Scan, plan_variants) on the host, with stand-in engines: no native call.

Two events with up to two prong slots on 16 x 16 maps in 8 x 8 tiles.  The stand-in embedders list the variants of a hit list as the
native ones do (every tile of every map that holds a hit, ascending; a pass's rows are the hits its variants keep); the stand-in head
writes each variant's (b, s, ty, tx) into the logits it returns, so a logits row can be traced to its index row."""
from types import SimpleNamespace

import pytest
import torch

from transformercvn.hip.occlusion import HitList, Scan, VariantPlan, plan_variants
from transformercvn.hip.runtime import LastForward

SHAPE, TILE, B, P, N_PRONGS = (16, 16), (8, 8), 2, 2, 3
MASK = torch.tensor([[True, True], [True, False]])
# (map, y, x): event 1 has all its hits in one tile, so its only variant is an empty map
EVENT_HITS = [(0, 1, 1), (0, 2, 9), (0, 12, 3), (1, 15, 15), (1, 14, 9)]
PRONG_HITS = [(0, 0, 0), (0, 9, 9), (1, 3, 12), (2, 8, 0), (2, 8, 7), (2, 15, 8)]
# variants by hand, ascending in (b, s, ty, tx): event maps are s = 0, prong maps (packed order) are (0, 1), (0, 2), (1, 1)
EVENT_INDEX = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 1, 1)]
PRONG_INDEX = [(0, 1, 0, 0), (0, 1, 1, 1), (0, 2, 0, 1), (1, 1, 1, 0), (1, 1, 1, 1)]


class Embedder:
    """Stand-in of an embedder engine: the variant list on the host, and counters of the calls."""

    def __init__(self, out_dim, always_unsorted=False):
        self.out_dim, self.always_unsorted = out_dim, always_unsorted
        self.variant_calls, self.builds, self.forwards, self.lists_seen = 0, [], [], []

    def occlusion_variants(self, coords, n_img, shape, tile, img_bs, max_pass, keep_map=None):
        self.variant_calls += 1
        self.lists_seen.append(coords.clone())
        c = coords.long()
        bad = bool(((c[:, 0] < 0) | (c[:, 0] >= n_img) | (c[:, 1] < 0) | (c[:, 1] >= shape[0]) | (c[:, 2] < 0) | (c[:, 2] >= shape[1])).any())
        unsorted = self.always_unsorted or bool((c[1:, 0] < c[:-1, 0]).any())
        tiles, rows = [], []
        if not (bad or unsorted):
            hits = [(int(i), int(y) // tile[0], int(x) // tile[1]) for i, y, x in c.tolist()]
            for i, ty, tx in sorted(set(hits)):
                b, s = img_bs[i].tolist()
                if keep_map is None or keep_map[b, s, ty // 2, tx // 2]:
                    tiles.append((i, b, s, ty, tx))
                    rows.append(sum(1 for h in hits if h[0] == i and h[1:] != (ty, tx)))
        V = len(tiles)
        bounds = [sum(rows[:min(k * max_pass, V)]) for k in range(-(-V // max_pass) + 1)]
        vimg = torch.tensor([t[0] for t in tiles], dtype=torch.int32)
        index = torch.tensor([t[1:] for t in tiles], dtype=torch.int32).reshape(V, 4)
        return VariantPlan(V, bounds, vimg, index, torch.empty(0), (n_img, *shape, *tile, max_pass)), unsorted, bad

    def occlusion_refine_variants(self, coords, n_img, shape, tile, img_bs, max_pass, keep_map):
        return self.occlusion_variants(coords, n_img, shape, tile, img_bs, max_pass, keep_map)

    def occlusion_build(self, plan, coords, values, first, count, out_coords, out_values):
        self.builds.append((first, count))

    def occlusion_forward(self, coords, values, nnz, n_img, out, log_pixels=0):
        self.forwards.append((nnz, n_img))
        out.zero_()


class Head:
    cfg = SimpleNamespace(event_classes=4, prong_classes=3)

    def __init__(self):
        self.passes = []

    def embed(self, rows, tok_row, batch, max_prongs, n_prongs, train, seed=0):
        return torch.zeros(batch, 1 + max_prongs, 8)

    def occlusion_pass(self, rows, tokens, tok_row, n_prongs, vimg, index, row_base, emb, col0, occ_ev, occ_pr):
        self.passes.append((index.shape[0], row_base, col0))
        occ_ev.copy_(index.float())
        i = index.long()
        occ_pr.copy_((((i[:, 0] * 10 + i[:, 1]) * 10 + i[:, 2]) * 10 + i[:, 3]).float().reshape(-1, 1, 1).expand_as(occ_pr))


def pixels(hits):
    coords = torch.tensor(hits, dtype=torch.int32)
    return SimpleNamespace(coords=coords, values=torch.arange(1.0, len(hits) + 1).reshape(-1, 1), value_mode=0)


def make_scan(maps="all", event_px=None, ev_engine=None):
    ev_engine, pr_engine, head = ev_engine or Embedder(12), Embedder(8), Head()
    last = LastForward(torch.zeros(B + N_PRONGS, 16), torch.zeros(B, 1 + P, dtype=torch.int32), B, P, N_PRONGS)
    scan = Scan(ev_engine, pr_engine, head, SHAPE, last, torch.zeros(B, 4), torch.zeros(B, P, 3), event_px or pixels(EVENT_HITS),
                pixels(PRONG_HITS), MASK, maps)
    return scan, ev_engine, pr_engine, head


def same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("index", "occluded_event_logits", "occluded_prong_logits"))


def test_merge_of_the_two_lists_is_ascending_and_rows_travel_with_their_index():
    scan, ev_engine, pr_engine, head = make_scan()
    assert [(l.engine, l.n_img, l.row_base, l.col0) for l in scan.lists] == [(ev_engine, B, 0, 0), (pr_engine, N_PRONGS, B, 4)]
    assert scan.lists[1].img_bs.tolist() == [[0, 1], [0, 2], [1, 1]]
    res = scan.level(TILE, 256)
    assert res.grid == (2, 2) and res.tile == TILE
    assert res.index.tolist() == [list(v) for v in sorted(EVENT_INDEX + PRONG_INDEX)]          # the two lists interleave: (0,0,*) (0,1,*) ..
    assert res.index.tolist() != [list(v) for v in EVENT_INDEX + PRONG_INDEX]
    assert torch.equal(res.occluded_event_logits, res.index.float())
    i = res.index.long()
    code = (((i[:, 0] * 10 + i[:, 1]) * 10 + i[:, 2]) * 10 + i[:, 3]).float()
    assert res.occluded_prong_logits.shape == (9, P, 3) and torch.equal(res.occluded_prong_logits[:, 1, 2], code)
    assert head.passes == [(4, 0, 0), (5, B, 4)]
    # one list alone is returned as the engine ordered it
    for maps, want in (("event", EVENT_INDEX), ("prongs", PRONG_INDEX)):
        assert make_scan(maps)[0].level(TILE, 256).index.tolist() == [list(v) for v in want]


def test_budget_below_the_number_of_variants_stops_before_any_pass():
    scan, ev_engine, pr_engine, head = make_scan()
    assert scan.level(TILE, 256, budget=8) is None
    assert ev_engine.variant_calls == pr_engine.variant_calls == 1
    assert not (ev_engine.builds or ev_engine.forwards or pr_engine.builds or pr_engine.forwards or head.passes)
    assert scan.level(TILE, 256, budget=9).num_variants == 9


def test_pass_size_does_not_change_the_result_and_empty_passes_skip_the_build_only():
    one, ev1, pr1, head1 = make_scan()
    big, ev256, pr256, head256 = make_scan()
    assert same(one.level(TILE, 1), big.level(TILE, 256))
    # one variant per pass: event 1's only variant keeps no hit (no build), yet goes through the embedder and the token path
    assert ev1.forwards == [(2, 1), (2, 1), (2, 1), (0, 1)] and ev1.builds == [(0, 1), (1, 1), (2, 1)]
    assert pr1.forwards == [(1, 1), (1, 1), (0, 1), (1, 1), (2, 1)] and pr1.builds == [(0, 1), (1, 1), (3, 1), (4, 1)]
    assert [p[0] for p in head1.passes] == [1] * 9
    assert ev256.forwards == [(6, 4)] and ev256.builds == [(0, 4)] and pr256.forwards == [(5, 5)] and head256.passes == [(4, 0, 0), (5, B, 4)]


def test_unsorted_list_with_hits_outside_the_maps_is_filtered_then_stably_sorted():
    g = torch.Generator().manual_seed(3)
    hits = EVENT_HITS + [(0, 2, 9), (2, 0, 0), (-1, 3, 3), (1, 16, 0), (0, 4, -2)]        # a second hit on (0, 2, 9), four rows to drop
    perm = torch.randperm(len(hits), generator=g)
    px = pixels([hits[k] for k in perm.tolist()])
    coords, values = px.coords.clone(), px.values.clone()
    keep = torch.tensor([0 <= i < B and 0 <= y < 16 and 0 <= x < 16 for i, y, x in px.coords.tolist()])
    order = torch.sort(px.coords[keep][:, 0], stable=True).indices
    want_coords, want_values = px.coords[keep][order], px.values[keep][order]

    engine = Embedder(12)
    lst = HitList(engine, px.coords, px.values, 0, B, torch.tensor([[0, 0], [1, 0]], dtype=torch.int32), 0, 0)
    cleaned, plan = plan_variants(lst, SHAPE, TILE, 256)
    assert engine.variant_calls == 2 and torch.equal(engine.lists_seen[0], coords) and torch.equal(engine.lists_seen[1], want_coords)
    assert torch.equal(cleaned.coords, want_coords) and torch.equal(cleaned.values, want_values)
    assert plan.index.tolist() == [list(v) for v in EVENT_INDEX]
    assert lst.coords is px.coords and torch.equal(px.coords, coords) and torch.equal(px.values, values)       # the input is as it was
    # a sorted, clean list is planned as it is
    again, _ = plan_variants(cleaned, SHAPE, TILE, 256)
    assert again is cleaned and engine.variant_calls == 3

    # inside a scan the cleaned list is kept for the later levels: one repeated variant call at the first level only
    scan, ev_engine, _, _ = make_scan("event", px)
    first = scan.level(TILE, 256)
    assert ev_engine.variant_calls == 2 and torch.equal(scan.lists[0].coords, want_coords)
    keep_map = torch.ones(B, 1 + P, 2, 2, dtype=torch.uint8)
    assert scan.level((4, 4), 256, keep_map).num_variants == 5 and ev_engine.variant_calls == 3
    assert first.index.tolist() == [list(v) for v in EVENT_INDEX] and torch.equal(px.coords, coords)

    with pytest.raises(RuntimeError, match="still unsorted after sorting"):
        make_scan("event", px, Embedder(12, always_unsorted=True))[0].level(TILE, 256)
