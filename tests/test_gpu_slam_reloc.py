"""GPU: retrieval-based relocalization and loop-closure edges in the SLAM driver (reference slam.py:159-214 feeding the
database, :216-290 RELOC).  Random-weight tracking is not deterministic, so the tracker is replaced by a stub that
forces each branch: (True, [], False) = new keyframe, (False, [], True) = tracking lost."""
import numpy as np
import pytest
import torch

from mast3r_slam import config, model as M, synthetic
from mast3r_slam.slam import SLAM, TRACKING

pytestmark = pytest.mark.gpu
H, W = 128, 256
NEW, LOST = (True, [], False), (False, [], True)


@pytest.fixture(scope="module")
def net(dev):
    return M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev)


def _frames(seeds):
    return [(0.1 * k, torch.from_numpy(synthetic.textured_image(H, W, s))) for k, s in enumerate(seeds)]


def _stub(s, plan):
    it = iter(plan)
    s.tracker.track = lambda frame, mast3r_match_fn=None: next(it)


def _edges(s):
    return list(zip(s.factor_graph.ii.tolist(), s.factor_graph.jj.tolist()))


def _sig64(feat):
    m = feat.detach().cpu().double().numpy().mean(axis=0)
    return m / np.sqrt((m * m).sum() + 1e-8)


def _assert_clear_best(query_feat, kf_feats, best):
    """Oracle similarities: `best` wins by more than 1e-4, so a pass cannot be a rounding accident."""
    sims = np.array([_sig64(f) @ _sig64(query_feat) for f in kf_feats])
    order = np.argsort(sims)[::-1]
    assert order[0] == best and sims[order[0]] - sims[order[1]] > 1e-4, sims


def _run(net, seeds, plan, cfg, **kw):
    config.set_config(cfg)
    s = SLAM(net, **kw)
    _stub(s, plan)
    solves = []
    orig = s.factor_graph.solve_GN_rays

    def solve():
        solves.append((len(s.keyframes), s.keyframes.last_keyframe().T_WC.clone()))
        orig()
    s.factor_graph.solve_GN_rays = solve
    s.run(_frames(seeds))
    return s, solves


def test_relocalization_succeeds_against_the_retrieved_keyframe(net, dev):
    try:
        s, solves = _run(net, [40, 41, 42, 40], [NEW, NEW, LOST], {"reloc": {"min_match_frac": 0.0}}, retrieval=True)
        kfs = s.keyframes
        assert len(kfs) == 4 and len(s.retrieval_db) == 4 and s.mode == TRACKING
        _assert_clear_best(kfs[3].feat, [kfs[i].feat for i in range(3)], 0)
        assert s.retrieval_candidates[3][0] == 0                           # the revisit's top candidate is A's keyframe
        assert (3, 0) in _edges(s)
        n_kf, pose = solves[-1]                                             # the relocalization solve: started at kf 0's pose
        assert n_kf == 4 and torch.equal(pose, kfs[0].T_WC)
        assert torch.equal(s.retrieval_db.signatures[3], s.retrieval_db.compute_signature(kfs[3].feat))
    finally:
        config.set_config({})


def test_relocalization_failure_pops_the_frame(net, dev):
    try:
        s, _ = _run(net, [40, 41, 42, 40], [NEW, NEW, LOST], {"reloc": {"min_match_frac": 1.01}}, retrieval=True)
        assert len(s.keyframes) == 3 and len(s.retrieval_db) == 3 and s.mode == TRACKING
        assert all(3 not in e for e in _edges(s))
        assert [kf.frame_id for kf in s.keyframes._frames] == [0, 1, 2]
    finally:
        config.set_config({})


@pytest.mark.parametrize("loop_closure", [True, False])
def test_loop_closure_edges(net, dev, loop_closure):
    try:
        s, _ = _run(net, [40, 41, 42, 43, 44, 40], [NEW] * 5, {"local_opt": {"min_match_frac": 0.0}}, retrieval=True,
                    loop_closure=loop_closure)
        kfs = s.keyframes
        assert len(kfs) == 6 and len(s.retrieval_db) == 6
        _assert_clear_best(kfs[5].feat, [kfs[i].feat for i in range(5)], 0)
        assert s.retrieval_candidates[5][0] == 0
        e = _edges(s)
        assert {(2, 5), (3, 5), (4, 5)} <= set(e)
        assert ((0, 5) in e) == loop_closure                                # outside the 3-keyframe window
    finally:
        config.set_config({})


def test_default_driver_is_unchanged(net, dev):
    """retrieval=None: a lost frame becomes a new keyframe at the last keyframe's pose, wired to its 3 predecessors."""
    try:
        s, _ = _run(net, [40, 41, 42, 40], [NEW, NEW, LOST], {"local_opt": {"min_match_frac": 0.0}})
        assert s.retrieval_db is None and s.retrieval_candidates == {}
        assert s.mode == TRACKING and len(s.keyframes) == 4
        assert _edges(s) == [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)]
    finally:
        config.set_config({})
