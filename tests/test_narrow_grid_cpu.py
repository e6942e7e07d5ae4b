"""tests/narrow_grid.py held to its word, without a GPU: the neighbour generator really puts every ordered pair of block kinds into one
wavefront on consecutive trips, at both parities, and the grid formulas restate what the launch code computes for the narrow geometries.

The check reads the batch as the kernels do -- block b is trip b // nwaves of wavefront b % nwaves -- and never asks the generator where
it believes it put something, except to compare."""
import importlib.util
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ng = _load("narrow_grid")


@pytest.mark.parametrize("nwaves", [1, 8, 16, 24])
def test_every_ordered_pair_sits_in_one_wavefront_on_consecutive_trips(nwaves):
    """1, 8, 16 wavefronts: the kernels under g1w1 and g1w8 (quad / generic: 8, fast: 16); 24: three workgroups of eight."""
    s = ng.neighbour_schedule(nwaves)
    assert len(s.kinds) % nwaves == 0 and s.n_trips % 2 == 0, "a full rectangle of blocks with an even trip count"
    assert set(s.kinds) == set(ng.KINDS), "every block kind occurs"
    pairs = ng.runs_in(s.kinds, nwaves, 2)
    for a in ng.KINDS:
        for b in ng.KINDS:
            assert pairs.get((a, b)) == {0, 1}, f"({a}, {b}) at parities {pairs.get((a, b))}"
    triples = ng.runs_in(s.kinds, nwaves, 3)
    for t in ng.triples_of(ng.KINDS):
        assert triples.get(t) == {0, 1}, f"{t} at parities {triples.get(t)}"
    # what the generator says it placed is where the batch has it
    for strip, places in s.placed.items():
        assert {t % 2 for _, t in places} == {0, 1}, strip
        for w, t in places:
            assert w < nwaves and tuple(s.kind_at(w, t + i) for i in range(len(strip))) == strip
    assert 4 * len(s.kinds) <= 4680, "no larger than the displaced corpus"


def test_triples_name_every_kind_in_the_middle():
    ts = ng.triples_of(ng.KINDS)
    assert {t[1] for t in ts} == set(ng.KINDS)
    assert all(len(t) == 3 and set(t) <= set(ng.KINDS) for t in ts)
    assert ("m17", "m17", "m17") in ts and ("reserved", "reserved", "reserved") in ts and ("parked", "parked", "parked") in ts


def test_runs_in_reads_the_batch_by_wavefront():
    kinds = ["a", "b", "c", "d", "e", "f"]                   # two wavefronts: a c e and b d f
    assert ng.runs_in(kinds, 2, 2) == {("a", "c"): {0}, ("b", "d"): {0}, ("c", "e"): {1}, ("d", "f"): {1}}
    assert ng.runs_in(kinds, 2, 3) == {("a", "c", "e"): {0}, ("b", "d", "f"): {0}}
    assert ng.runs_in(kinds, 1, 2) == {("a", "b"): {0}, ("b", "c"): {1}, ("c", "d"): {0}, ("d", "e"): {1}, ("e", "f"): {0}}


def test_grids_and_trips_of_the_narrow_geometries():
    """The table of the module: g1w8 is one workgroup of 8 (quad, generic) or 16 (fast) wavefronts; g3w8 up to three of them; g1w1 one
    wavefront for the quad and the fast kernel."""
    assert ng.expected_grid("quad", 640, "g1w8") == (1, 512) and ng.trips("quad", 640, 1, 512) == 20
    assert ng.expected_grid("fast", 640, "g1w8") == (1, 1024) and ng.trips("fast", 640, 1, 1024) == 40
    assert ng.expected_grid("generic", 640, "g1w8") == (1, 512) and ng.trips("generic", 640, 1, 512) == 80
    assert ng.expected_grid("quad", 4680, "g1w8") == (1, 512) and ng.trips("quad", 4680, 1, 512) == 147
    assert ng.expected_grid("quad", 4680, "g1w1") == (1, 64) and ng.trips("quad", 4680, 1, 64) == 1170
    assert ng.expected_grid("fast", 4680, "g1w1") == (1, 64) and ng.trips("fast", 4680, 1, 64) == 4680
    assert ng.expected_grid("quad", 132, "g3w8") == (3, 512) and ng.trips("quad", 132, 3, 512) == 2
    assert ng.expected_grid("quad", 33, "g3w8") == (2, 512) and ng.expected_grid("quad", 1, "g3w8") == (1, 512)
    assert ng.expected_grid("fast", 17, "g3w8") == (2, 1024) and ng.expected_grid("generic", 200, "g3w8") == (3, 512)
    for env, cfg in ng.GEOMETRIES.values():
        assert set(env) <= set(ng.GEOMETRY_KNOBS) and env["EPPK_MAX_CU"] == str(cfg["max_cu"]) and env["EPPK_MAX_WG_PER_CU"] == "1"
        assert int(env.get("EPPK_QUAD_THREADS", 512)) == cfg["quad"] and int(env.get("EPPK_FAST_THREADS", 1024)) == cfg["fast"]
