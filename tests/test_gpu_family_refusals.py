"""The capability matrix of the families that run their own kernels ("The family table"; kFamilies of csrc/api_common.h), cell
by cell through the public ABI: every entry a family lacks returns MIVI_ERR_UNSUPPORTED with "<entry>: not supported on the <family name>",
before it reads a buffer.  Only refused cells are called (with placeholder buffers); the per-family test files exercise the others."""
import numpy as np
import pytest

import advancedvi_jl_amd as avi
from advancedvi_jl_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 0x38BEF07CF9CC549D
D, M = 8, 4
MC = avi.MonteCarloEntropy.code

LOWRANK = "low-rank family (MIVI_LOWRANK)"
REALNVP = "RealNVP family (MIVI_REALNVP)"
NSF = "neural spline flow family (MIVI_NSF)"
BLOCKDIAG = "block-diagonal family (MIVI_BLOCKDIAG)"

CONTEXTS = {
    LOWRANK: lambda: avi.MiviContext(np.float32, avi.LOWRANK, D, M, avi.ClosedFormEntropy.code, SEED, rank=2),
    REALNVP: lambda: avi.MiviContext(np.float32, avi.REALNVP, D, M, MC, SEED, flow=((4,), 2)),
    NSF: lambda: avi.MiviContext(np.float32, avi.NSF, D, M, MC, SEED, flow=((4,), 2, 4, 3.0)),
    BLOCKDIAG: lambda: avi.MiviContext(np.float32, avi.BLOCKDIAG, D, M, avi.ClosedFormEntropy.code, SEED, block=4),
}

# capability -> (the families it refuses, one representative entry: (ctx, P) -> status, the entry as the message names it)
PARTIALS = "mivi_estimate_partials"
PROX = "mivi_prox_scale_entropy (the reference has no ProximalLocationScaleEntropy method for it)"
STD = "mivi_logpdf with std_dev (the family has no square scale to standardise by)"
CLIP = "mivi_clip_scale (ClipScale has no method for a family without a scale)"
MANY = "mivi_optimize_loop_many (the family has no launch-free loop)"
SCHEDULE = "mivi_logreg_set_batch_schedule"
BASE = "mivi_set_base_dist with a non-normal base"
BASE_FLOW = "mivi_set_base_dist with a non-normal base (the flow's base is the standard normal)"


def _raw(call):
    return lambda ctx, P, buf: call(ctx.lib, ctx.h, P)


def _wrapped(call):
    def run(ctx, P, buf):
        with pytest.raises(avi.MiviError) as e:
            call(ctx, buf)
        return e.value.status
    return run


CALLS = {
    PARTIALS: _raw(lambda lib, h, P: lib.mivi_estimate_partials(h, P, 0, P)),
    PROX: _raw(lambda lib, h, P: lib.mivi_prox_scale_entropy(h, P, 0.1, None, 0)),
    STD: _raw(lambda lib, h, P: lib.mivi_logpdf(h, P, P, 1, P, P)),
    CLIP: _raw(lambda lib, h, P: lib.mivi_clip_scale(h, P, 1e-5)),
    MANY: _wrapped(lambda ctx, buf: ctx.optimize_loop_many(buf[:2 * ctx.params_len], 2, 2, 0, 0)),
    SCHEDULE: _wrapped(lambda ctx, buf: ctx.set_batch_schedule(np.zeros((1, 2), np.int64), likeadj=1.0)),
    BASE: _raw(lambda lib, h, P: lib.mivi_set_base_dist(h, 1, 0.0)),
}
CALLS[BASE_FLOW] = CALLS[BASE]

# The R cells of the matrix: (family, entry text).  A cell marked loose is one of the two low-rank messages that were hand-written before
# the table gave them the uniform form: entry and family are asserted as substrings.
CELLS = [(f, PARTIALS) for f in (LOWRANK, REALNVP, NSF, BLOCKDIAG)]
CELLS += [(f, PROX) for f in (LOWRANK, REALNVP, NSF)]
CELLS += [(f, STD) for f in (LOWRANK, REALNVP, NSF)]
CELLS += [(f, CLIP) for f in (REALNVP, NSF)]
CELLS += [(f, MANY) for f in (LOWRANK, REALNVP, NSF, BLOCKDIAG)]
CELLS += [(f, SCHEDULE) for f in (REALNVP, NSF, BLOCKDIAG)]
CELLS += [(LOWRANK, BASE), (REALNVP, BASE_FLOW), (NSF, BASE_FLOW), (BLOCKDIAG, BASE)]
LOOSE = {(LOWRANK, MANY): ("mivi_optimize_loop_many", "low-rank family"), (LOWRANK, BASE): ("mivi_set_base_dist", "low-rank family (MIVI_LOWRANK)")}


@pytest.mark.parametrize("family", list(CONTEXTS))
def test_refused_cells_name_the_entry_and_the_family(family):
    ctx = CONTEXTS[family]()
    try:
        buf = ctx.empty(4 * (D * D + D * M) + 2 * ctx.params_len + 64)
        P = ctx._p(buf)
        cells = [entry for f, entry in CELLS if f == family]
        assert cells and len(CELLS) == len(set(CELLS)) == 4 + 3 + 3 + 2 + 4 + 3 + 4   # (the R cells of the matrix, row by row)
        for entry in cells:
            assert CALLS[entry](ctx, P, buf) == _lib.ERR_UNSUPPORTED, (family, entry)
            msg = ctx.lib.mivi_last_error(ctx.h).decode()
            if (family, entry) in LOOSE:
                assert all(part in msg for part in LOOSE[(family, entry)]), (family, entry, msg)
            else:
                assert msg == entry + ": not supported on the " + family, (family, entry, msg)
    finally:
        ctx.close()

