"""AdaptiveBinding.get_w (adaptive.py:32-60) restated for BOTH matching types, on the soft-DTW of oracle/adaptive_oracle.py:

  dtw_image    cost = batch_cdist(tree.df.images, inputs.traj_seq, 'mean')            (adaptive.py:42-44)
  dtw_latent   cost = batch_cdist(tree.df.e_g_prime, inputs.enc_traj_seq, 'mean')     (adaptive.py:45-47)

then, for both,  w = normalize(soft_dtw(cost.detach() / temp, end_ind), 1)  (adaptive.py:50-58), depth-first, float64 inside the lattice.
The cost is formed in the dtype of what is passed in: float32 images give the bits of oracle.adaptive_oracle.get_w (pinned by
tests/test_adaptive_latent_cpu.py), float64 latents a float64 cost.  oracle/adaptive_oracle.get_w itself asserts 'dtw_image'; the GPU
tests put `patched_get_w` in its place for a 'dtw_latent' model (oracle/gcp_model_oracle.py calls it as AD.get_w)."""
import torch

from oracle import adaptive_oracle as A

TEMP = "tree_module.tree_modules.0.binding.temp"


def get_w(hp, sd, nodes_df, frames, end_ind):
    """nodes_df [B, N, ...] depth-first: the decoded images ('dtw_image') or the node latents e_g_prime ('dtw_latent'); frames
    [B, T, ...]: traj_seq or enc_traj_seq.  Returns (w [B, N, T] float32, cost [B, N, T]) like oracle.adaptive_oracle.get_w.  With a
    learned temperature that requires grad the division by it stays in the graph (adaptive.py:19-21, :51)."""
    assert hp.matching_type in ("dtw_image", "dtw_latent")
    cost = A.hack_weights_df(A.batch_cdist(nodes_df, frames, reduction="mean"), hp)
    temp = sd[TEMP]
    if hp.learn_matching_temp and temp.requires_grad:
        return A.normalize(A.soft_dtw_autograd(cost.detach() / temp, end_ind), 1), cost
    w = A.soft_dtw((cost.detach() / temp.detach()).numpy(), end_ind.numpy())
    return A.normalize(torch.from_numpy(w), 1), cost


def patched_get_w(latents_df, enc_traj_seq):
    """what a test assigns to oracle.adaptive_oracle.get_w for a 'dtw_latent' model: the call's image arguments are ignored, the cost
    is taken between the given latents, detached as adaptive.py:51 detaches the cost (the latents of a model do not depend on its
    matching, so those of an earlier pass with the same parameters and inputs are the ones this pass computes)"""
    lat, enc = latents_df.detach(), enc_traj_seq.detach()

    def fn(hp, sd, images_df, traj_seq, end_ind):
        assert hp.matching_type == "dtw_latent"
        return get_w(hp, sd, lat, enc, end_ind)
    return fn


def top_two_gap(w, dim):
    """smallest difference between the largest and the second largest entry along `dim`, over all the other indices"""
    top = torch.topk(w.double(), 2, dim=dim).values
    return float((top.select(dim, 0) - top.select(dim, 1)).min())
