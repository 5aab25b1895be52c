"""The distance field and the Voronoi cells where the lower-envelope stacks run deep: k_distance_minplus (vrc_distance.hip) and
k_fracture_minplus (vrc_fracture.hip) at 128^3 (stacks in LDS), 256^3 (stacks in device memory) and 512^3 (the line loop's
second step on a device of 256 compute units), with the z passes, select, dilate / erode and clearance reading what they
leave.  The scenes, the references and the geometry they reach are tests/envelope_cases.py's, held to their conditions in
tests/test_volume_envelope_cases_host.py.  No reference is a lower-envelope walk: scipy's feature transform with the squared
distance recomputed in int64, the closed form of a union of products, a packed min-plus in numpy, the closed form of a
product grid.  Every comparison is exact."""

import numpy as np
import pytest

import clearance_model
import components_model
import distance_model as model
import envelope_cases as cases
import posed_cases
import stamp_model
from test_gpu_volume_fracture import device_cells
from test_gpu_volume_large import same
from volume_support import affine_records, differing, labels_of

pytestmark = pytest.mark.gpu
NONE = cases.NONE


def upload(vol):
    """the dense array as a volume: its solid voxels set, or, when most are solid, its empty ones cleared out of a full one"""
    import cpuvoxelraycaster_amd as vrc
    S = vol.shape[0]
    volume = vrc.VoxelVolume(S.bit_length() - 1)
    if 2 * int(vol.sum(dtype=np.int64)) > vol.size:
        volume.fillBoxes([[0, 0, 0, S, S, S]])
        volume.setVoxels(np.argwhere(vol == 0), False)
    else:
        volume.setVoxels(np.argwhere(vol))
    return volume


def upload_products(sets):
    """the union of the products A x B x C by slabs: a product is the slabs of A less the slabs of the complements of B and C"""
    import cpuvoxelraycaster_amd as vrc
    S = len(sets[0][0])
    volume, part = vrc.VoxelVolume(S.bit_length() - 1), vrc.VoxelVolume(S.bit_length() - 1)
    for A, B, C in sets:
        fill, clear = cases.product_boxes(A, B, C)
        part.fillBoxes([[0, 0, 0, S, S, S]], False)
        part.fillBoxes(fill)
        if len(clear):
            part.fillBoxes(clear, False)
        volume.copyRegion(part, (0, 0, 0), (S, S, S), (0, 0, 0), vrc.capi.VRC_COPY_OR)
    part.close()
    assert volume.solidCount() == cases.product_count(sets)
    return volume


def upload_scene(name, S):
    vol = cases.scene(name, S)
    volume = upload_products(cases.axis_sets(S)) if name == "products" else upload(vol)
    assert np.array_equal(volume.download(), vol), (name, S)
    return volume


def check_stats(field, want, features, what):
    s = field.stats
    assert (int(s.features), int(s.max_d2), tuple(int(v) for v in s.argmax), int(s.reserved)) == (features, want[0], want[1], 0), what


# ---- the distance field at 128^3 and 256^3 ----------------------------------------------------------------------------

# the two fields of the slant at 256^3 come last: the clearance test below reads them again
FIELDS = [(name, S, to_empty) for S in cases.SIZES for name in ("ball", "products", "slant") for to_empty in (False, True)]


@pytest.mark.parametrize("name,S,to_empty", FIELDS)
def test_distance_field_of_a_scene(built, name, S, to_empty):
    """download() and the stats of both `outside` values against the feature transform; at 256^3 a shell of the field through
    select as well"""
    volume = upload_scene(name, S)
    inside = cases.scene_field(name, S, to_empty)
    features = int(cases.features_of(cases.scene(name, S), to_empty).sum())
    for outside in (False, True):
        D = model.open_border(inside) if outside else inside
        field = volume.distanceField(to_empty, outside)
        same(field.download(), D, (name, S, to_empty, outside))
        check_stats(field, model.stats(D), features, (name, S, to_empty, outside))
        if S == 256 and not outside:
            m = model.stats(D)[0]
            lo, hi = max(1, m // 8), max(1, m // 2)                          # a shell between an eighth and half of the largest value
            K = model.select(D, lo, hi)
            assert 0 < int(K.sum()) < S ** 3, (lo, hi)
            shell = field.select(lo, hi)
            same(shell.download(), K, ("select", name, to_empty, lo, hi))
            shell.close()
        field.close()
    volume.close()


def test_dilate_and_erode_the_ball_complement_at_128(built):
    """dilate(3) and erode(3) through the field: distance_model's rule (select 0 <= D <= 9) over the feature transform --
    the model's own field of 128^3 does not fit a test of a few seconds"""
    vol = cases.scene("ball", 128)
    grown = upload(vol)
    grown.dilate(3)
    want = (vol != 0) | (model.select(cases.scene_field("ball", 128, False), 0, 9) != 0)
    assert int(want.sum()) > int(vol.sum())
    same(grown.download() != 0, want, "dilate")
    grown.close()
    shrunk = upload(vol)
    shrunk.erode(3)
    want = (vol != 0) & (model.select(cases.scene_field("ball", 128, True), 0, 9) == 0)
    assert 0 < int(want.sum()) < int(vol.sum())
    same(shrunk.download() != 0, want, "erode")
    shrunk.close()


# ---- the distance field at 512^3 --------------------------------------------------------------------------------------

def halves(got, want):
    """where a 512^3 field differs, by the iteration of the line loop that wrote it: the y pass takes the lines x >= 256 in its
    second step, the x pass the lines y >= 256"""
    h = got.shape[0] // 2
    return {"x < %d" % h: int((got[:h] != want[:h]).sum()), "x >= %d" % h: int((got[h:] != want[h:]).sum()),
            "y < %d" % h: int((got[:, :h] != want[:, :h]).sum()), "y >= %d" % h: int((got[:, h:] != want[:, h:]).sum())}


def second_step_or_skip():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cases.line_steps(9, cus) < 2:
        pytest.skip("%d compute units launch %d workgroups for the 4096 wanted at 512^3: no second step" % (cus, cases.minplus_groups(9, cus)))
    assert cases.minplus_groups(9, cus) < 4096


def test_distance_field_at_512_takes_a_second_line(built):
    """512^3, the union of products against its closed form, the faces as walls and open: every workgroup of the min-plus
    passes takes a second 64 lines on the stacks of the first"""
    second_step_or_skip()
    S = 512
    sets = cases.axis_sets(S)
    volume = upload_products(sets)
    features = cases.product_count(sets)
    want = cases.products_field(sets)
    for outside in (False, True):
        if outside:
            cases.open_border_in_place(want)
        field = volume.distanceField(False, outside)
        got = field.download()
        stats = field.stats
        field.close()                                                        # before the next one is made
        if not np.array_equal(got, want):
            where = np.argwhere(got != want)
            raise AssertionError("outside %d: %d voxels differ %s, the first at %s" % (outside, len(where), halves(got, want), where[:5].tolist()))
        m, arg = cases.stats_of_finite(want)
        assert (int(stats.features), int(stats.max_d2), tuple(int(v) for v in stats.argmax)) == (features, m, arg), outside
        del got
    volume.close()


# ---- the cells at 128^3 -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["given", "shuffled"])
@pytest.mark.parametrize("name", ["slant", "products"])
def test_cells_at_128(built, name, order):
    """the cell of every voxel against the packed min-plus over whole lines, unlimited and within 10 voxels"""
    S = 128
    sites = cases.scene_sites(name, S)
    if order == "shuffled":
        sites = cases.shuffled(sites)
    P = cases.packed_field(S, sites)
    for r in (None, 10):
        want = cases.cells_of_packed(P, NONE if r is None else r * r)
        same(device_cells(S, sites, r), want, (name, order, r))


# ---- the cells at 256^3 -----------------------------------------------------------------------------------------------

RADIUS_256 = 5


@pytest.mark.parametrize("name,order", [("slant", "given"), ("slant", "shuffled"), ("products", "shuffled")])
def test_cells_at_256_within_a_radius(built, name, order):
    """the stacks in device memory, as deep as without the cut-off (the last pass alone applies it), against the windowed packed
    min-plus.  Only a shuffled order can tell the strict pop rule from the distance field's: in dense order the middle site of
    three whose parabolas meet never has the lowest index"""
    S, r = 256, RADIUS_256
    sites = cases.scene_sites(name, S)
    if order == "shuffled":
        sites = cases.shuffled(sites)
    want = cases.packed_cells(S, sites, r * r, r)
    assert int((want != NONE).sum()) > S ** 3 // 16
    same(device_cells(S, sites, r), want, (name, order, r))


def test_cells_of_a_product_grid_with_triples_at_256(built):
    """the grid and its triples off the grid, unlimited, against the closed form with the triples' sites by brute force"""
    S = 256
    g = cases.grid_sites(S, cases.GRID_COUNTS[S])
    want = cases.grid_cells(g, S)
    got = device_cells(S, g.sites)
    won = cases.tie_won_triples(g, S)
    assert len(won) >= 5
    centres = tuple(g.centres[won].T)
    assert np.array_equal(got[centres], want[centres]), "a voxel that only the tie gives to the middle site of a triple"
    same(got, want, "grid")


# ---- the cells at 512^3 -----------------------------------------------------------------------------------------------

def test_cells_of_a_product_grid_at_512(built):
    """SAMPLED: VoxelLabels has no dense read-out, and at() of all 2^27 voxels would move 1.5 GiB of coordinates; the cell is
    read through the piece at a lattice of stride 8 and at random voxels, 2^21 probes, three quarters of them beyond x = 256
    or y = 256, where the line loop's second step writes.  The closed form of the grid is the reference."""
    import cpuvoxelraycaster_amd as vrc
    second_step_or_skip()
    S = 512
    g = cases.grid_sites(S, cases.GRID_COUNTS[S])
    # the probes, and every voxel within 4 of the centre of a triple: the voxels the strict pop rule decides
    around = (g.centres[:, None, :] + np.indices((9, 9, 9)).reshape(3, -1).T[None] - 4).reshape(-1, 3)
    xyz = np.concatenate([cases.probes_512(), around.astype(np.uint32)])
    late = (xyz[:, 0] >= 256) | (xyz[:, 1] >= 256)
    assert len(xyz) >= 1 << 21 and 2 * int(late.sum()) >= len(xyz)
    won = g.centres[cases.tie_won_triples(g, S)]
    assert ((won[:, 0] >= 256) | (won[:, 1] >= 256)).sum() >= 3 and len(won) >= 5
    want = cases.grid_cells_at(g, S, xyz)
    empty = vrc.VoxelVolume(9)
    labels = empty.fracture(g.sites, 6, True)
    empty.close()
    at = labels.at(xyz)
    assert (at != NONE).all()
    got = labels.pieceSites()[at]
    labels.close()
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), int(late[bad].sum()), xyz[bad[:5]].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


# ---- clearance over the 256^3 field -----------------------------------------------------------------------------------

@pytest.mark.parametrize("to_empty", [False, True])
def test_clearance_over_the_slant_at_256(built, to_empty):
    """twenty boxes of a 32^3 labelling moved about the 256^3 slant + specks field, to the solid and to the empty"""
    S = 256
    debris, offsets = cases.clearance_case(S)
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == len(offsets)
    maps = [(list(stamp_model.IDENTITY[0]), [-(int(v) << 17) for v in o]) for o in offsets]
    boxes = np.concatenate([rec["lo"].astype(np.int64) + offsets, rec["hi"].astype(np.int64) + offsets], axis=1).astype(np.uint32)
    D = cases.scene_field("slant", S, to_empty)
    sets = posed_cases.posed_point_sets(ids, maps, boxes, S)
    want = clearance_model.records_of(sets, D)
    assert [w[0] for w in want] == rec["voxels"].tolist()
    volume = upload_scene("slant", S)
    field = volume.distanceField(to_empty, False)
    volume.close()
    labels = labels_of(debris, 6)
    got = clearance_model.tuples(labels.clearance(affine_records(maps), field, boxes))
    assert got == want, differing(got, want)
    field.close()
    labels.close()
