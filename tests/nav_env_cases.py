"""Cases shared by tests/test_nav_env_cpu.py and tests/test_gpu_nav_env.py: the hand-built steps in the 9-room maze and a small control
configuration in the reference's format."""
import textwrap

import numpy as np

from video_gcp_amd import nav_env as NE
from video_gcp_amd import nav_layout as NL

R = NL.ROBOT_SIZE
POST = NL.DOOR_SIZE / 2                     # a door post of the 9-room maze's centre room: (+-1 / 6, +-POST)

# the centre room is [-1/6, 1/6]^2: open doors in its left and right walls (x = +-1/6, |y| < POST), closed ones above and below
# (y = +-1/6, |x| <= POST).  (name, start, end, blocked) in table coordinates
HAND_CASES = [
    ("free step inside a room", (0.0, 0.0), (0.05, 0.03), False),
    ("through an open door's centre", (0.1, 0.0), (0.23, 0.0), False),
    ("head-on across a wall, both ends farther than r from it", (0.1, 0.1), (0.23, 0.1), True),
    ("ends closer than r to a wall without crossing", (0.1, 0.1), (0.155, 0.1), True),
    ("through a closed door", (0.0, 0.1), (0.0, 0.23), True),
    ("past a door post at just under r", (0.1, POST - R + 1e-4), (0.23, POST - R + 1e-4), True),
    ("past a door post at just over r", (0.1, POST - R - 1e-4), (0.23, POST - R - 1e-4), False),
    ("leaving the table", (0.45, 0.3), (0.55, 0.3), True),
]


def hand_case_rows():
    """[(name, state float32 [3], action float32 [2], blocked)] in the environment's units, and the zero action"""
    rows = []
    for k, (name, p, q, blocked) in enumerate(HAND_CASES):
        s = np.concatenate([NE.table2env(np.array(p)), [np.float32(0.25 * k - 1.0)]]).astype(np.float32)
        a = (NE.table2env(np.array(q)) - s[:2]).astype(np.float32)
        rows.append((name, s, a, blocked))
    rows.append(("a zero action", np.array([1.0, -2.0, 0.7], dtype=np.float32), np.zeros(2, dtype=np.float32), False))
    return rows



CONF = textwrap.dedent('''
    import os.path
    from blox import AttrDict
    from gcp.planning.infra.agent.benchmarking_agent import BenchmarkAgent
    from gcp.planning.infra.envs.miniworld_env.multiroom3d.multiroom3d_env import {env_cls}
    from gcp.planning.planner_policy import ImageCEMPolicy
    from gcp.planning.cem.sampler import ImageHierarchicalTreeCEMSampler
    from gcp.planning.cem.cem_planner import HierarchicalImageCEMPlanner
    from gcp.planning.cem.cost_fcn import ImageLearnedCostEstimate
    from experiments.prediction.base_configs import gcp_tree as base_conf

    agent = AttrDict(type=BenchmarkAgent, env=({env_cls}, dict({env_params})), T={T}, image_height=32, image_width=32,
                     start_goal_confs=os.environ['GCP_DATA_DIR'] + '/start_goal')
    h_config = AttrDict(base_conf.model_config)
    h_config.update(dict(state_dim=2, ngf=16, max_seq_len=12, hierarchy_levels=4, nz_mid_lstm=64, n_lstm_layers=2, nz_mid=32, nz_enc=32,
                         nz_vae=32, regress_length=True, attach_state_regressor=True, attach_inv_mdl=True,
                         inv_mdl_params=AttrDict(n_actions=2, use_convs=False, build_encoder=False), untied_layers=True,
                         decoder_distribution='discrete_logistic_mixture'))
    h_config.pop("add_weighted_pixel_copy")
    cem_params = AttrDict(prune_final=True, horizon=12, action_dim=32, verbose=False, n_level_hierarchy=4,
                          sampler=ImageHierarchicalTreeCEMSampler, cost_fcn=ImageLearnedCostEstimate,
                          cost_config=AttrDict(checkpt_path=os.environ['GCP_EXP_DIR'] + '/prediction/weights'),
                          n_iters=3, batch_size=3, sampling_rates_per_layer=[3, 3])
    policy = AttrDict(type=ImageCEMPolicy, params=h_config, checkpt_path=cem_params.cost_config.checkpt_path,
                      cem_planner=HierarchicalImageCEMPlanner, cem_params=cem_params, replan_interval=agent.T + 2,
                      closed_loop_execution=True)
    config = AttrDict(current_dir=os.path.dirname(os.path.realpath(__file__)), start_index=0, end_index=99, agent=agent, policy=policy,
                      save_format=['raw'], data_save_dir=os.environ['GCP_EXP_DIR'] + '/control', split_train_val_test=False,
                      traj_per_file=1)
''')
