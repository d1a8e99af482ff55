"""The variant lists of the explanation scans, looked at directly: tcvn_occlusion_variants / _refine_variants / _curve_variants and
their build passes through ctypes, no model.  Everything is integer bookkeeping, so every comparison with the host reference
(occlusion_reference.list_reference: filter the image's rows, prefix sums of the counts, a Python sort for the ranking) is torch.equal:
the header words (V, unsorted, bad, nh), every pass bound, vimg, index, the curves' rank, and for every pass the rows of out_coords and
out_values.  Values are distinct floats with 3 channels, so a swapped row shows.  The shapes are the smallest that cross each loop
boundary of the kernels: the 1 024-cell chunks of the compaction, the 256-hit chunks and 64-lane waves of the build, more than 1 024
maps, pass boundaries that are exact multiples of max_pass, and the T + 1-th prefix entry of a 4 096-tile sort."""
import ctypes as C

import pytest
import torch

import occlusion_reference as R

pytestmark = pytest.mark.gpu

GUARD = 4                       # rows behind a pass's hit list that the build must leave alone
_cache = {}


def distinct_values(nnz):
    return torch.arange(3 * nnz, dtype=torch.float32).reshape(nnz, 3) + 0.5          # exact in float32 far beyond these sizes


def random_hits(img, n, shape, g):
    y = torch.randint(0, shape[0], (n,), generator=g)
    x = torch.randint(0, shape[1], (n,), generator=g)
    return torch.stack((torch.full((n,), img), y, x), 1)


def carries_list():
    """5 maps of 40x40: map 0 holds 600 hits (three 256-hit chunks of the build), map 2 none, map 4 one; two hits of map 0 sit on one
    pixel with different values."""
    if "carries" not in _cache:
        g = torch.Generator().manual_seed(11)
        shape = (40, 40)
        c0 = random_hits(0, 600, shape, g)
        c0[300, 1:] = c0[17, 1:]
        coords = torch.cat((c0, random_hits(1, 50, shape, g), random_hits(3, 70, shape, g), torch.tensor([[4, 39, 39]]))).int()
        assert int((coords[:, 0] == 0).sum()) == 600 and torch.equal(coords[300, 1:], coords[17, 1:])
        _cache["carries"] = (coords, distinct_values(coords.shape[0]), 5, shape)
    return _cache["carries"]


MAPS5 = torch.tensor([[0, 0], [0, 1], [0, 2], [1, 0], [1, 1]], dtype=torch.int32)


def device_list(coords, n_img, shape, tile, img_bs, max_pass, keep_map=None, curve=None):
    """One variant-list call -> (host words, vimg, index, workspace, build geometry, rank or None, the coords on the device), the
    outputs pre-filled with -7."""
    from transformercvn.hip._lib import lib
    from transformercvn.hip.native import ptr, stream_ptr
    (H, W), (th, tw) = shape, tile
    Ht, Wt = R.grid_of(shape, tile)
    dev = torch.device("cuda")
    d_coords, d_bs = coords.to(dev).contiguous(), img_bs.to(dev).contiguous()
    rank = None
    if curve is None:
        rows, geometry = n_img * Ht * Wt, (n_img, H, W, th, tw, max_pass)
        need = lib.tcvn_occlusion_workspace_bytes(*geometry)
    else:
        relevance, steps, mode = curve
        rows, geometry = n_img * (steps + 1), (n_img, H, W, th, tw, steps, mode, max_pass)
        need = lib.tcvn_occlusion_curve_workspace_bytes(n_img, H, W, th, tw, steps, max_pass)
        rank = torch.full(tuple(relevance.shape), -1, dtype=torch.int32, device=dev)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    vimg = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    index = torch.full((rows, 4), -7, dtype=torch.int32, device=dev)
    words = 4 + -(-rows // max_pass) + 1
    host = (C.c_int64 * words)(*([-7] * words))
    head = (ptr(d_coords), coords.shape[0], n_img, H, W, th, tw, ptr(d_bs))
    tail = (max_pass, ptr(vimg), ptr(index), ptr(ws), ws.numel(), host, words, stream_ptr())
    if curve is not None:
        d_rel = relevance.to(dev).contiguous()
        rc = lib.tcvn_occlusion_curve_variants(*head, ptr(d_rel), relevance.shape[0], relevance.shape[1] - 1, steps, mode, ptr(rank),
                                               *tail)
    elif keep_map is not None:
        d_keep = keep_map.to(dev).contiguous()
        B, S, pHt, pWt = keep_map.shape
        rc = lib.tcvn_occlusion_refine_variants(*head, ptr(d_keep), B, S - 1, pHt, pWt, *tail)
    else:
        rc = lib.tcvn_occlusion_variants(*head, *tail)
    assert rc == 0
    return list(host), vimg, index, ws, geometry, rank, d_coords


def check_list(coords, values, n_img, shape, tile, img_bs, max_pass, keep_map=None, curve=None, build=True):
    """The list call and every build pass against the host reference; -> the reference (for what a case asserts on top)."""
    from transformercvn.hip._lib import lib
    from transformercvn.hip.native import ptr, stream_ptr
    ref = R.list_reference(coords, n_img, shape, tile, img_bs, max_pass, keep_map, curve)
    host, vimg, index, ws, geometry, rank, d_coords = device_list(coords, n_img, shape, tile, img_bs, max_pass, keep_map, curve)
    V = ref["header"][0]
    print(f"V {host[0]} unsorted {host[1]} bad {host[2]} nh {host[3]} passes {-(-V // max_pass)} (reference {ref['header']})")
    assert host[:4] == ref["header"]
    assert host[4:] == ref["bounds"]
    assert torch.equal(vimg[:V].cpu(), ref["vimg"]) and bool((vimg[V:] == -7).all())
    assert torch.equal(index[:V].cpu(), ref["index"]) and bool((index[V:] == -7).all())
    if curve is not None:
        assert torch.equal(rank.cpu(), ref["rank"])
    if not build:
        return ref
    assert host[1] == 0 and host[2] == 0
    bounds = ref["bounds"]
    d_values = values.to(d_coords.device).contiguous()
    fn = lib.tcvn_occlusion_build_pass if curve is None else lib.tcvn_occlusion_curve_build_pass
    for k in range(-(-V // max_pass)):
        first, count, n = k * max_pass, min(max_pass, V - k * max_pass), bounds[k + 1] - bounds[k]
        if n == 0:
            continue
        out_coords = torch.full((n + GUARD, 3), -7, dtype=torch.int32, device=d_coords.device)
        out_values = torch.full((n + GUARD, values.shape[1]), -7.0, device=d_coords.device)
        assert fn(ptr(d_coords), ptr(d_values), coords.shape[0], values.shape[1], *geometry, ptr(vimg), ptr(ws), ws.numel(), first, count,
                  ptr(out_coords), ptr(out_values), n + GUARD, stream_ptr()) == 0
        want_coords, want_values = R.pass_reference(ref, coords, values, first, count)
        assert want_coords.shape[0] == n
        assert torch.equal(out_coords[:n].cpu(), want_coords), f"pass {k}: coords"
        assert torch.equal(out_values[:n].cpu(), want_values), f"pass {k}: values"
        assert bool((out_coords[n:] == -7).all()) and bool((out_values[n:] == -7.0).all()), f"pass {k}: rows behind the list"
    return ref


@pytest.mark.parametrize("max_pass", [7, 256])
def test_carries_of_the_compaction_and_the_build(max_pass):
    coords, values, n_img, shape = carries_list()
    ref = check_list(coords, values, n_img, shape, (2, 2), MAPS5, max_pass)
    assert n_img * 400 > 1024 and ref["header"][0] > 256                       # two chunks of cells; more than one pass at 256 too
    assert 2 not in ref["vimg"].tolist() and ref["vimg"].tolist().count(4) == 1


@pytest.mark.parametrize("max_pass", [1, 4, 5, 12, 256])
def test_pass_boundaries(max_pass):
    """3 maps of 8x8 in tiles of (4, 4), every tile occupied: V = 12; exact multiples, a remainder, and V < max_pass."""
    g = torch.Generator().manual_seed(5)
    corners = torch.tensor([[i, ty * 4, tx * 4] for i in range(3) for ty in range(2) for tx in range(2)])
    coords = torch.cat((corners, random_hits(0, 9, (8, 8), g), random_hits(2, 5, (8, 8), g)))
    coords = coords[torch.sort(coords[:, 0], stable=True).indices].int()
    ref = check_list(coords, distinct_values(coords.shape[0]), 3, (8, 8), (4, 4), MAPS5[:3], max_pass)
    assert ref["header"][0] == 12


@pytest.mark.parametrize("tile", [(2, 2), (1, 1)])
def test_many_maps(tile):
    """1 100 maps of 2x2, a hit (or two) in every map but each third one: the first-hit prologue takes two chunks.  One tile a map
    leaves no variant a hit; tiles of one pixel make the builds read the first-hit table on both sides of entry 1 024."""
    g = torch.Generator().manual_seed(7)
    imgs = torch.tensor([i for i in range(1100) if i % 3 != 2 for _ in range(1 + i % 2)])
    coords = torch.stack((imgs, torch.randint(0, 2, imgs.shape, generator=g), torch.randint(0, 2, imgs.shape, generator=g)), 1).int()
    img_bs = torch.stack((torch.arange(1100), torch.zeros(1100, dtype=torch.long)), 1).int()
    ref = check_list(coords, distinct_values(coords.shape[0]), 1100, (2, 2), tile, img_bs, 256)
    assert ref["header"][0] >= 1100 - 1100 // 3 and (tile == (1, 1)) == (ref["header"][3] > 0)
    assert (ref["header"][0] == 1100 - 1100 // 3) == (tile == (2, 2))


@pytest.mark.parametrize("channels", [1, 4])
def test_build_pass_at_other_channel_counts(channels):
    """The detector tests' lists (40 x 28 maps of 0, 1, 255, 256 and 700 hits, pixels listed twice) with one and four value channels per
    hit: the build pass copies hit * channels + c."""
    from test_detector_gpu import SHAPE, synthetic_list
    coords, values = synthetic_list(channels)
    assert values.shape[1] == channels
    ref = check_list(coords, values, 5, SHAPE, (8, 7), MAPS5, 3)
    assert ref["header"][0] > 3 and ref["header"][3] > 0


def test_empty_list():
    ref = check_list(torch.empty(0, 3, dtype=torch.int32), torch.empty(0, 3), 2, (8, 8), (4, 4), MAPS5[:2], 4, build=False)
    assert ref["header"] == [0, 0, 0, 0] and ref["bounds"][0] == 0 and not any(ref["bounds"])


def test_flags():
    """An unsorted list sets only the first flag; a hit with y = H, one with x = -1 and one with img = n_img set only the second."""
    shape, n_img = (8, 8), 2
    unsorted = torch.tensor([[0, 1, 1], [1, 2, 2], [0, 5, 5], [1, 7, 7]], dtype=torch.int32)
    ref = check_list(unsorted, distinct_values(4), n_img, shape, (4, 4), MAPS5[:2], 4, build=False)
    assert ref["header"][1:3] == [1, 0]
    for outside in ([0, 8, 1], [0, 1, -1], [2, 1, 1]):
        coords = torch.tensor([[0, 1, 1], [0, 5, 5], outside, [1, 2, 2]], dtype=torch.int32)
        coords = coords[torch.sort(coords[:, 0], stable=True).indices]
        ref = check_list(coords, distinct_values(4), n_img, shape, (4, 4), MAPS5[:2], 4, build=False)
        assert ref["header"][1:3] == [0, 1], outside


def test_refinement():
    """The carries list under a seeded keep_map of the 10x10 parent grid; then one map named (-1, 0): it has no variant, and the lists
    of the other maps are what they were."""
    coords, values, n_img, shape = carries_list()
    keep_map = (torch.rand(2, 3, 10, 10, generator=torch.Generator().manual_seed(13)) < 0.5).to(torch.uint8)
    ref = check_list(coords, values, n_img, shape, (2, 2), MAPS5, 7, keep_map=keep_map)
    flat = R.list_reference(coords, n_img, shape, (2, 2), MAPS5, 7)
    assert 0 < ref["header"][0] < flat["header"][0]
    unnamed = MAPS5.clone()
    unnamed[1] = torch.tensor([-1, 0])
    ref2 = check_list(coords, values, n_img, shape, (2, 2), unnamed, 7, keep_map=keep_map)
    assert 1 in ref["vimg"].tolist() and 1 not in ref2["vimg"].tolist()
    others = [v for v in range(ref["header"][0]) if ref["vimg"][v] != 1]
    assert torch.equal(ref["index"][others], ref2["index"]) and len(others) == ref2["header"][0]
    assert all(torch.equal(ref["rows"][v], ref2["rows"][j]) for j, v in enumerate(others))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("steps", [1, 4, 64])
def test_curves_small(steps, mode):
    """2 maps of 6x6 in tiles of (2, 2): T = 9, sorted as 16 keys.  The relevance has ties, 0.0 against -0.0 and negative values; one
    tile of each map is unoccupied; 64 steps are more than the occupied tiles."""
    g = torch.Generator().manual_seed(3)
    shape, tile = (6, 6), (2, 2)
    hits = torch.cat((random_hits(0, 40, shape, g), random_hits(1, 25, shape, g)))
    hits = hits[~((hits[:, 1] // 2 == 1) & (hits[:, 2] // 2 == 2))].int()            # tile (1, 2) stays empty
    rel = torch.tensor([[0.5, -0.0, 0.0], [0.5, -1.25, 9.0], [-1.25, 0.0, 0.25]]).expand(2, 1, 3, 3).contiguous()
    assert torch.signbit(rel[0, 0, 0, 1]) and not torch.signbit(rel[0, 0, 0, 2])
    img_bs = torch.tensor([[0, 0], [1, 0]], dtype=torch.int32)
    ref = check_list(hits, distinct_values(hits.shape[0]), 2, shape, tile, img_bs, 5, curve=(rel, steps, mode))
    assert ref["header"][0] == 2 * (steps + 1) and int((ref["rank"] >= 0).sum()) == 16
    assert ref["rank"][0, 0].tolist() == [[0, 3, 4], [1, 6, -1], [7, 5, 2]]


@pytest.mark.parametrize("mode", [0, 1])
def test_curves_full_sort(mode):
    """1 map of 64x64 in tiles of (1, 1): T = 4 096, the limit; the prefix loop writes entry T in a chunk of its own."""
    g = torch.Generator().manual_seed(17)
    shape = (64, 64)
    hits = random_hits(0, 3000, shape, g).int()
    rel = (torch.randint(-8, 8, (1, 1, 64, 64), generator=g).float() / 4).contiguous()
    ref = check_list(hits, distinct_values(3000), 1, shape, (1, 1), MAPS5[:1], 4, curve=(rel, 10, mode))
    assert ref["header"][0] == 11
