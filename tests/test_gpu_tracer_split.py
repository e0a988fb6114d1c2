"""The tracer's split launches (csrc/tracer.hip), which no other test reaches - the widest tracer batch elsewhere is 67:
Tracer::launch_walk issues a sample-major walk of more than 32 768 realizations as several launches with offset output
pointers, and Tracer::run stages host fluxes of more than 2^24 values in pieces.  Every test reads PMC_COUNT_TRACER_SPLIT:
the split must have happened in the wide batch and must not have happened in its narrow twin, so that a retuned threshold
fails the test instead of quietly returning it to the single launch.  Run with -m gpu on an MI355X.

- the walk: one particle at (0.5, 0.5, 0) of the unit box under the box_ln2 flux of tracer_cases.exact_paths scaled by
  1 + b / 65 536 in realization b (every realization has its own bits), 32 768 + 3 realizations: T, x_exit within TOL_K of
  the numpy twin and exit_face, status, nsteps equal to it for EVERY realization, rows 32 767 and 32 768 - the two sides of
  the cut - bit for bit the single-realization runs, and the same batch through device memory bit for bit the host one;
- the staged upload: the hex1 case (240 faces, 64 particles), 2^24 / 240 + 2 = 69 907 realizations, fluxes the oracle flux
  times 1 + 1e-3 (b mod 7): the host arrays are 134 MB of fluxes and 197 MB of results (under the 1 GiB the issue allows, so
  no other mesh is needed).  Realizations 0, per - 1, per and the last one bit for bit the single-realization runs; and,
  since realizations with the same b mod 7 carry the same flux, every row bit for bit row b mod 7 - a piece written at the
  wrong offset cannot hide between the four compared rows.  Each staged piece is itself walked in three launches
  (69 905 = 2 x 32 768 + 4 369).

Seeded in a scratch copy: the output offset `o` dropped from the second launch of launch_walk fails all three tests below
(test_gpu_tracer.py does not notice it: its widest batch is 67).  Measured on the MI355X: T and x_exit of all 32 771
realizations equal the twin's bit for bit (tolerance 8.8e-12); each of the three tests takes under a second."""
import numpy as np
import pytest

import tracer_cases as tc
from parelagmc_amd.fe import tracer as tr

pytestmark = pytest.mark.gpu

KEYS = ("T", "exit_face", "status", "nsteps", "x_exit")
WALK_LIMIT = 32768            # realizations per sample-major launch (blockIdx.y)
STAGE_VALUES = 1 << 24        # flux values per staged piece


def _splits(ctx):
    from parelagmc_amd import capi
    return ctx.lib.pmc_solve_path_count(capi.PMC_COUNT_TRACER_SPLIT)


def _same(a, b, rows_a, rows_b):
    return all(np.array_equal(a[k][rows_a], b[k][rows_b]) for k in KEYS)


@pytest.fixture(scope="module")
def box(gpu_ctx):
    from parelagmc_amd import capi
    path = next(p for p in tc.exact_paths() if p.name == "box_ln2")
    nb = WALK_LIMIT + 3
    u = path.u[None, :] * (1.0 + np.arange(nb)[:, None] / 65536.0)
    t = capi.Tracer(gpu_ctx, path.mesh, path.x0, np.zeros(1, np.int32))
    before = _splits(gpu_ctx)
    host = t.Run(u)
    moved = _splits(gpu_ctx) - before
    yield dict(path=path, u=u, t=t, host=host, moved=moved)
    t.close()


def test_walk_of_more_than_one_launch_matches_the_twin(gpu_ctx, box):
    path, u, t, got = box["path"], box["u"], box["t"], box["host"]
    assert box["moved"] == 1, "the walk of 32 771 realizations was not split"
    ref = tr.trace(path.mesh, u, path.x0, np.zeros(1, np.int32))
    for key in ("status", "exit_face", "nsteps"):
        assert np.array_equal(got[key], ref[key]), key
    assert (got["status"] == t.EXITED).all() and (got["exit_face"] == path.face).all() and (got["nsteps"] == 1).all()
    dT = np.abs(got["T"] - ref["T"]) / ref["T"]
    dx = np.abs(got["x_exit"] - ref["x_exit"]).max(axis=2)
    print(f"tracer split walk: max relative difference T {dT.max():.3g}, x_exit {dx.max():.3g} (tolerance {tc.TOL_K:.3g}); "
          f"first launch {dT[:WALK_LIMIT].max():.3g}, second {dT[WALK_LIMIT:].max():.3g}")
    assert dT.max() <= tc.TOL_K and dx.max() <= tc.TOL_K
    # both sides of the cut against launches of their own; the narrow twin does not split
    before = _splits(gpu_ctx)
    for j in (0, WALK_LIMIT - 1, WALK_LIMIT, WALK_LIMIT + 2):
        assert _same(got, t.Run(u[j:j + 1]), [j], [0]), j
    assert _same(got, t.Run(u[:WALK_LIMIT]), slice(0, WALK_LIMIT), slice(None))
    assert _splits(gpu_ctx) == before, "a batch of at most 32 768 realizations was split"


def test_split_walk_in_device_memory_has_the_same_bits(gpu_ctx, box):
    u, t, host = box["u"], box["t"], box["host"]
    before = _splits(gpu_ctx)
    dev = t.Run(gpu_ctx.array(u), nbatch=len(u))
    assert _splits(gpu_ctx) - before == 1
    assert _same(host, {k: v.download().reshape(host[k].shape) for k, v in dev.items()}, slice(None), slice(None))
    before = _splits(gpu_ctx)
    narrow = t.Run(gpu_ctx.array(u[:32]), nbatch=32)
    assert _splits(gpu_ctx) == before
    assert _same(host, {k: v.download().reshape(host[k][:32].shape) for k, v in narrow.items()}, slice(0, 32), slice(None))


def test_staged_upload_in_pieces_matches_single_realizations(gpu_ctx):
    from parelagmc_amd import capi
    c, flux = tc.case("hex1"), tc.oracle_flux("hex1")[0]
    per = STAGE_VALUES // c.mesh.n_face
    nb = per + 2
    assert per > WALK_LIMIT and nb * c.mesh.n_face * 8 < 2 ** 30
    u = flux[None, :] * (1.0 + 1e-3 * (np.arange(nb) % 7))[:, None]
    t = capi.Tracer(gpu_ctx, c.mesh, c.x0, c.elem0)
    try:
        before = _splits(gpu_ctx)
        got = t.Run(u)
        # the upload in two pieces, and the walk of the first piece in three launches
        assert _splits(gpu_ctx) - before == 2, "the fluxes were not staged in pieces"
        assert (got["status"] == t.EXITED).all()
        before = _splits(gpu_ctx)
        for j in (0, WALK_LIMIT - 1, WALK_LIMIT, 2 * WALK_LIMIT, per - 1, per, nb - 1):
            assert _same(got, t.Run(u[j:j + 1]), [j], [0]), j
        first = t.Run(u[:7])
        assert _splits(gpu_ctx) == before, "a narrow batch was split"
        rows = np.arange(nb) % 7
        for k in KEYS:
            assert np.array_equal(got[k], first[k][rows]), k
    finally:
        t.close()
