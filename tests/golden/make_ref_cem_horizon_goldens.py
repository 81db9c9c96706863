"""Golden vectors of the REFERENCE's horizon cap, produced by executing /root/reference/gcp/planning/cem/cem_planner.py
(CEMPlanner.__call__ with _rollout's _cap_to_horizon, :115-122,151-155, and _get_action_plan, :143-149) in the build container.

Run from the repo root:  python tests/golden/make_ref_cem_horizon_goldens.py  ->  tests/golden/ref_cem_horizon.npz   (arrays only)

The set-up is make_ref_cem_loop_goldens.py's: the stub simulator of planner_stubs.py (rollout lengths 3 .. 6 of 6 steps, a function of the
candidate), the reference's own EuclideanPathLength, the Gaussian numbers of every `sampler.sample` recorded (the same for every case).  Cases: horizon 2 (below every
rollout's length), 4 (between the lengths), 6 (the longest rollout) and 9 (above all of them), each with use_inferred_actions True (the
action plan is the final rollout's actions, capped) and False (the best sample itself, uncapped).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ref_cem_loop_goldens import install_all, NoiseTap   # noqa: E402
from planner_stubs import flat_stub_rollout                    # noqa: E402

STEPS, AD, N_ITERS, BATCH, ELITE_FRAC = 6, 3, 3, 20, 0.2


def main():
    AttrDict, ParamDict, C, S, P = install_all()
    out = {}

    class FlatStubSim:
        def rollout(self, state, goal, samples, max_seq_len):
            preds, lat = flat_stub_rollout(samples, max_seq_len, np.float64)
            return AttrDict(predictions=preds, states=[p.copy() for p in preds], actions=[p[1:] - p[:-1] for p in preds], latents=lat)

    cases = [(h, inferred) for h in (2, 4, 6, 9) for inferred in (True, False)]
    out["cases"] = np.array([[h, int(i)] for h, i in cases])
    out["shape"] = np.array([STEPS, AD, N_ITERS, BATCH])
    out["elite_frac"] = np.array([ELITE_FRAC])
    goal = np.linspace(-0.5, 0.5, AD)
    out["goal"] = goal
    for ci, (horizon, inferred) in enumerate(cases):
        hp = dict(horizon=horizon, action_dim=AD, n_iters=N_ITERS, batch_size=BATCH, max_rollout_bs=100, elite_frac=ELITE_FRAC,
                  cost_fcn=C.EuclideanPathLength, dense_cost=True, final_step_cost_weight=2.0, sampler=S.FlatCEMSampler,
                  sampler_clip_val=np.inf, initial_std=0.6, max_seq_len=STEPS, use_inferred_actions=inferred)
        np.random.seed(10)                                               # one stream for every case: the unit numbers are stored once
        planner = P.CEMPlanner(dict(hp), FlatStubSim())
        picks, lens = [], []
        orig = planner._get_best_rollouts

        def tapped(rollouts, goal_state, samples, _o=orig, _p=picks, _l=lens, _pl=planner):
            r = _o(rollouts, goal_state, samples)
            _p.append((np.asarray(_pl._cost_fcn(rollouts.predictions, goal_state), dtype=np.float64), np.asarray(r[4]), np.asarray(r[2], dtype=np.float64)))
            _l.append(np.array([len(p) for p in rollouts.predictions]))
            return r
        planner._get_best_rollouts = tapped
        with NoiseTap() as tap:
            pred, actions, latents, score = planner(None, goal)
        for it in range(N_ITERS):
            scores, idx, best_scores = picks[it]
            assert len(np.unique(scores)) == len(scores), "tied scores: argsort order would be implementation-defined"
            assert np.array_equal(out.setdefault(f"it{it}_eps", tap.eps[it]), tap.eps[it])
            out[f"c{ci}_it{it}_scores"], out[f"c{ci}_it{it}_elite_idx"], out[f"c{ci}_it{it}_elite_scores"] = scores, idx, best_scores
            out[f"c{ci}_it{it}_lengths"] = lens[it]                       # of the capped rollouts the cost read
            d = planner._logs[0][it].dists
            out[f"c{ci}_it{it}_mean"], out[f"c{ci}_it{it}_std"] = np.asarray(d.mean), np.asarray(d.std)
        out[f"c{ci}_plan_pred"], out[f"c{ci}_plan_actions"], out[f"c{ci}_plan_latents"] = np.asarray(pred), np.asarray(actions), np.asarray(latents)
        out[f"c{ci}_plan_score"] = np.asarray(score, dtype=np.float64).reshape(1)
    path = os.path.join(HERE, "ref_cem_horizon.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
