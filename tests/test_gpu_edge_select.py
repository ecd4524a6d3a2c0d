"""The exact fan-out on the device (csrc/edge_select.hip) against tests/edge_select_ref.py, bit for bit: kernel, sampler, models
(data and helpers: test_gpu_edge_sample_model.py's for gat and sage max, test_gpu_edge_sample_val_model.py's for gcn and sage mean)."""
import numpy as np
import pytest

import edge_sample_ref as ref
import edge_sample_val_ref as vref
import edge_select_ref as sel
import test_gpu_edge_sample_model as walk
import test_gpu_edge_sample_val_model as summed
from guarded import Guarded

pytestmark = pytest.mark.gpu

ctx = walk.ctx                      # a context per test: its timers are this test's


@pytest.mark.parametrize("row0,col0", [(0, 0), (1000, 7)])
@pytest.mark.parametrize("force_stream", [False, True])
@pytest.mark.parametrize("keep", [1.0, 0.5])
@pytest.mark.parametrize("k", [1, 10, 64, 100])
def test_select_equals_the_restatement(pkg, ctx, k, keep, force_stream, row0, col0):
    ops, reg, n = pkg.ops, pkg.ops.EDGE_SELECT_REG_ENTRIES, sel.N_ROWS
    assert ctx.lib.mggcn_edge_sample_select_reg_entries() == reg
    ip, ix = sel.graph(k, reg)
    want = sel.select(ip, ix, k, keep, row0, col0, sel.SEED, sel.EPOCH)
    assert (want == sel.t_keep(keep)).sum() > 3 and (want < sel.t_keep(keep)).sum() > 3      # both branches of the contract
    import torch
    ip_d, ix_d = (torch.from_numpy(a.view(np.int32)).cuda() for a in (ip, ix))
    kw = dict(col0=col0, seed=sel.SEED, epoch=sel.EPOCH, force_stream=force_stream)

    def run(r0, r1):
        out = Guarded(r1 - r0, 1, 1, output=True)
        ops.edge_sample_select(ctx, r1 - r0, ip_d[r0:], ix_d, k, sel.t_keep(keep), out.t[out.start:], row0=row0 + r0, **kw)
        ctx.sync()
        out.check_guards(f"rows {r0}:{r1}")                         # nothing past n_rows (or in front) is written
        return out.logical_bits().ravel()

    with pytest.raises(ValueError, match="k must be"):
        ops.edge_sample_select(ctx, n, ip_d, ix_d, 0, sel.t_keep(keep), ip_d)
    whole = run(0, n)
    np.testing.assert_array_equal(whole, want)
    np.testing.assert_array_equal(run(0, n), whole)                 # a second call: the same bits
    np.testing.assert_array_equal(np.concatenate([run(0, 13), run(13, n)]), whole)      # two calls over a split of the rows


@pytest.mark.parametrize("rescale", [None, "row"])
def test_sampler_draws_the_restated_exact_pair(pkg, ctx, rescale):
    F_T = walk._csr(pkg, walk._sage_data(pkg)[0], walk.SAGE_N)
    F = F_T.transpose()
    sampler = pkg.edge_sampler(F, F_T, fanout=3, rescale=rescale, exact=True)
    seen = []
    for epoch in (0, 1):
        pair = sampler.draw(ctx, sel.SEED, epoch)
        thr = sel.select(F.indptr, F.indices, 3, 1.0, seed=sel.SEED, epoch=epoch)
        np.testing.assert_array_equal(sampler._thr.cpu().numpy().view(np.uint32), thr)
        for M, S, t in zip((F, F_T), pair, (0, 1)):
            for got, want in zip(S.numpy(), ref.sample(M.indptr, M.indices, thr, t, seed=sel.SEED, epoch=epoch)[1:]):
                np.testing.assert_array_equal(got, want)
            if rescale:                                             # test_gpu_edge_sample_val.py's bars for "row"
                scale = sampler._scale.cpu().numpy()
                r64, whole, nothing, length = vref.row_factors(F.indptr, F.indices, F.data, thr, seed=sel.SEED, epoch=epoch)
                assert (np.abs(scale - r64) <= 2.0 * length * 2.0 ** -24 * r64).all() and (scale[whole] == 1.0).all()
                want_v = vref.sample_val(M.indptr, M.indices, M.data, thr, t, scale, True, seed=sel.SEED, epoch=epoch)[3]
                np.testing.assert_array_equal(S.values_numpy().view(np.uint32), want_v.view(np.uint32))
        seen.append(pair[0].numpy()[1].tobytes())
    assert seen[0] != seen[1] and "sample-select" in ctx.timers and sampler.thr_host is None


MODELS = {"v1": (walk, {}), "v2": (walk, {}), "dot": (walk, {}), "sage": (walk, {}),
          "sage-mean-row": (summed, dict(edge_rescale="row")), "gcn-inverse": (summed, dict(edge_rescale="inverse"))}


@pytest.mark.parametrize("name", list(MODELS))
def test_models_train_on_the_exact_fan_out(pkg, ctx, name):
    mod, kw = MODELS[name]
    make = lambda **more: mod._make(pkg, name.split("-")[0], **kw, **more)[:3]
    ctor = {} if name in ("v1", "v2", "dot") else dict(fanout_exact=True)      # gat is switched by set_sampling alone
    plain, X, Y = make()
    want = [plain.train_step(ctx, X, Y, *walk.ADAM) for _ in range(3)]
    same, X, Y = make(fanout=10 ** 6, **ctor)                       # no row reaches it: every threshold 0xFFFFFFFF, every factor 1
    same.set_sampling(fanout=10 ** 6, seed=walk.SEED, exact=None if ctor else True)
    assert [same.train_step(ctx, X, Y, *walk.ADAM) for _ in range(3)] == want and "sample-select" in ctx.timers
    assert all((a == b).all() for a, b in zip(mod._param_bits(same), mod._param_bits(plain)))
    assert same.sample_exact and (same.sampler._thr.cpu().numpy().view(np.uint32) == 0xFFFFFFFF).all()
    two, X, Y = make(fanout=2, **ctor)                              # a real fan-out: finite, another loss, epoch 0 replays
    two.set_sampling(fanout=2, exact=None if ctor else True)
    first = two.train_step(ctx, X, Y, *walk.ADAM)
    assert np.isfinite(first[0]) and first[0] != want[0][0] and two.sample_epoch == 1
    again, X, Y = make()
    again.set_sampling(fanout=2, seed=0, epoch=0, exact=True)
    assert again.train_step(ctx, X, Y, *walk.ADAM) == first
