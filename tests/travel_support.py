"""What the travel-field tests share (tests/test_gpu_volume_travel.py, tests/test_gpu_volume_sweep_large.py): one field of
the device held against an expected one.  The library is imported inside volume_support's functions, so collecting needs no
built library."""
import numpy as np

import travel_model as model
from volume_support import all_coordinates, volume_of

NONE = model.NONE


def check_field(field, T, n_seeds, connectivity, what, step_limit=0, with_at=True, tight=False):
    """download(), at() of everything, stats, bytes(), depth and connectivity against an expected field.  The sweeps issued
    stay within the library's hard loop bound, 8^depth + 1 or step_limit + 2; `tight`: within max T + 2 as well (the
    counters are read back every few sweeps, so on a field of a handful of steps a few more than that are issued)."""
    S = T.shape[0]
    depth = S.bit_length() - 1
    got = field.download()
    assert got.dtype == np.uint32 and got.shape == (S, S, S)
    assert np.array_equal(got, T), (what, int((got != T).sum()), np.argwhere(got != T)[:4].tolist())
    if with_at:
        at = field.at(all_coordinates(S))
        assert np.array_equal(at[:S ** 3].reshape(S, S, S), T), what
        assert (at[S ** 3:] == NONE).all(), what
    seeds, reached, m, arg = model.stats(T, n_seeds)
    s = field.stats
    assert (int(s.seeds), int(s.reached), int(s.max_steps), tuple(int(v) for v in s.argmax), int(s.reserved)) == (seeds, reached, m, arg, 0), what
    assert int(s.sweeps) <= min(step_limit + 2 if step_limit else 8 ** depth + 1, 8 ** depth + 1), (what, int(s.sweeps))
    assert not tight or int(s.sweeps) <= m + 2, (what, int(s.sweeps), m)
    assert (int(s.sweeps) == 0) == (n_seeds == 0), (what, int(s.sweeps))
    assert field.bytes() == 4 * S ** 3 and field.depth == depth and field.data_ptr() != 0 and field.connectivity == connectivity


def run_case(vol, seeds, connectivity, through_empty, what, step_limit=0, with_at=True, volume=None, seed_volume=None, tight=False):
    """one field of the device against the model; returns the model's field"""
    depth = vol.shape[0].bit_length() - 1
    T = model.field(vol, seeds, connectivity, through_empty, step_limit)
    own = volume is None
    volume = volume_of(vol, depth) if volume is None else volume
    seed_volume = volume_of(seeds, depth) if seed_volume is None else seed_volume
    field = volume.travelField(seed_volume, connectivity, through_empty, step_limit)
    check_field(field, T, int(model.seeds_in_m(vol, seeds, through_empty).sum()), connectivity, what, step_limit, with_at, tight)
    field.close()
    if own:
        volume.close()
        seed_volume.close()
    return T
