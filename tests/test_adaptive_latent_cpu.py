"""CPU: matching_type = 'dtw_latent' (adaptive.py:45-47) and tied tree levels in the hyper-parameters and the conf loader, and the
restatement of AdaptiveBinding.get_w the GPU tests compare with (tests/adaptive_latent_refs.py) against the oracle's own get_w."""
import textwrap

import pytest
import torch

import adaptive_latent_refs as LR
from helpers import make_inputs


def test_hparams_accept_dtw_latent():
    import video_gcp_amd as V
    from video_gcp_amd.hparams import GCPHParams
    hp = GCPHParams(matching_type="dtw_latent")
    assert hp.adaptive and hp.matching_type == "dtw_latent"
    assert V.config("c5s", matching_type="dtw_latent", untied_layers=False).adaptive
    with pytest.raises(AssertionError):
        GCPHParams(matching_type="dtw_pixels")


def test_conf_on_the_adaptive_base_config_is_tied_attentive_and_takes_dtw_latent(tmp_path):
    """base_configs/gcp_adaptive.py sets neither untied_layers (hyperparameters.py:117: False) nor the mixture head; a room conf sets
    the head, pops the pixel-copy stream, and here asks for the latent cost"""
    from video_gcp_amd import conf_loader as CL
    (tmp_path / "conf.py").write_text(textwrap.dedent('''
        from blox import AttrDict
        from experiments.prediction.base_configs import gcp_adaptive as base_conf
        configuration = AttrDict(base_conf.configuration)
        configuration.update({'batch_size': 8, 'lr': 1e-3})
        model_config = AttrDict(base_conf.model_config)
        model_config.update({'hierarchy_levels': 8, 'decoder_distribution': 'discrete_logistic_mixture',
                             'matching_type': 'dtw_latent'})
        model_config.pop("add_weighted_pixel_copy")
    '''))
    hp, trainer, _ = CL.load_conf(str(tmp_path), max_seq_len=200)
    assert hp.matching_type == "dtw_latent" and hp.adaptive
    assert hp.untied_layers is False and hp.attentive_inference is True
    assert hp.learn_matching_temp is False and hp.decoder_distribution == "discrete_logistic_mixture"
    assert trainer["model"] == "tree" and hp.batch_size == 8 and hp.hierarchy_levels == 8
    # the same conf without the key keeps the base config's image cost, tied as well
    (tmp_path / "conf.py").write_text(textwrap.dedent('''
        from blox import AttrDict
        from experiments.prediction.base_configs import gcp_adaptive as base_conf
        configuration = AttrDict(base_conf.configuration)
        model_config = AttrDict(base_conf.model_config)
        model_config.pop("add_weighted_pixel_copy")
    '''))
    hp = CL.load_conf(str(tmp_path), max_seq_len=12, img_sz=32)[0]
    assert hp.matching_type == "dtw_image" and hp.untied_layers is False
    # ... and one that asks for untied levels gets them
    (tmp_path / "conf.py").write_text("configuration = {}\nmodel_config = {'matching_type': 'dtw_latent', 'untied_layers': True}\n")
    hp = CL.load_conf(str(tmp_path), max_seq_len=12, img_sz=32)[0]
    assert hp.matching_type == "dtw_latent" and hp.untied_layers is True


def _case(learn_temp, T=12):
    import video_gcp_amd as V
    hp = V.config("c5s", max_seq_len=T, learn_matching_temp=learn_temp)
    sd = V.init_params(hp, seed=1)
    sd[LR.TEMP].fill_(0.3)
    g = torch.Generator().manual_seed(3)
    N = hp.n_nodes
    images = torch.rand(2, N, 3, 32, 32, generator=g) * 2 - 1
    traj = torch.rand(2, T, 3, 32, 32, generator=g) * 2 - 1
    traj[0, 2] = images[0, 4]                                   # one exact match
    end = torch.tensor([T - 1, 2])
    return hp, sd, images, traj, end


@pytest.mark.parametrize("T", [12, 7])
def test_image_form_has_the_bits_of_the_oracles_get_w(T):
    from oracle import adaptive_oracle as A
    hp, sd, images, traj, end = _case(False, T)
    w, cost = LR.get_w(hp, sd, images, traj, end)
    w_ref, cost_ref = A.get_w(hp, sd, images, traj, end)
    assert w.dtype == torch.float32 and torch.equal(w, w_ref) and torch.equal(cost, cost_ref)
    # with a learned temperature: the same values and the same derivative
    hp, sd, images, traj, end = _case(True, T)
    grads = []
    for fn in (LR.get_w, A.get_w):
        leaf = dict(sd)
        leaf[LR.TEMP] = sd[LR.TEMP].clone().requires_grad_(True)
        w_t, _ = fn(hp, leaf, images, traj, end)
        assert w_t.requires_grad
        grads.append((w_t.detach(), torch.autograd.grad((w_t * torch.arange(T)[None, None]).sum(), leaf[LR.TEMP])[0]))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert torch.allclose(grads[0][0], w, atol=2e-6)


def test_latent_form_is_soft_dtw_of_the_latent_cost():
    """'dtw_latent': the mean squared distance over nz_enc between node and frame latents, the same soft-DTW and normalisation behind
    it; columns beyond end_ind are zero, the others distributions over the nodes; the patched oracle entry ignores the images"""
    import dataclasses
    from oracle import adaptive_oracle as A
    hp, sd, images, traj, end = _case(False)
    hp = dataclasses.replace(hp, matching_type="dtw_latent")
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(2, hp.n_nodes, hp.nz_enc, generator=g, dtype=torch.float64)
    enc = torch.randn(2, hp.max_seq_len, hp.nz_enc, generator=g, dtype=torch.float64)
    w, cost = LR.get_w(hp, sd, lat, enc, end)
    want = ((lat[:, :, None] - enc[:, None]) ** 2).mean(-1)
    assert cost.dtype == torch.float64 and torch.allclose(cost, want, rtol=1e-12, atol=1e-12)
    w2 = A.normalize(torch.from_numpy(A.soft_dtw((want / 0.3).numpy(), end.numpy())), 1)
    assert torch.allclose(w, w2, atol=1e-6)
    for b in range(2):
        e = int(end[b])
        assert torch.allclose(w[b, :, :e + 1].sum(0), torch.ones(e + 1), atol=1e-5)
        assert float(w[b, :, e + 1:].abs().sum()) == 0.0
    with pytest.raises(AssertionError):
        A.get_w(hp, sd, images, traj, end)                      # the oracle's own entry states the image form only
    w3, _ = LR.patched_get_w(lat, enc)(hp, sd, images, traj, end)
    assert torch.equal(w3, w)
    assert LR.top_two_gap(torch.tensor([[[0.5, 0.2], [0.1, 0.7]]]), 2) == pytest.approx(0.3)


def test_oracle_model_runs_the_latent_form_through_the_patched_entry(monkeypatch):
    """the oracle's model (gcp_model_oracle calls AD.get_w) with the latent restatement in place: the matching differs from the image
    form's, everything in front of it does not; the latents gcp_model_oracle computes are the ones the closure holds"""
    import video_gcp_amd as V
    from oracle import adaptive_oracle as A
    from oracle import gcp_model_oracle as O
    hp = V.config("c5s", max_seq_len=7)
    hpl = V.config("c5s", max_seq_len=7, matching_type="dtw_latent")
    sd = V.init_params(hp, seed=1, randomize_affine=True)
    sd[LR.TEMP].fill_(0.3)
    inputs, noise, _ = make_inputs(hp, seed=4, variant="B")
    ref = O.forward(sd, hp, inputs, noise=noise, training_bn=True)
    lat = O._bf_to_df(ref["tree_bf"]["e_g_prime"], hp.hierarchy_levels)
    monkeypatch.setattr(A, "get_w", LR.patched_get_w(lat, ref["inputs"]["enc_traj_seq"]))
    out = O.forward(sd, hpl, inputs, noise=noise, training_bn=True)
    assert torch.equal(out["tree_bf"]["e_g_prime"], ref["tree_bf"]["e_g_prime"])
    assert torch.equal(out["tree_bf"]["images"], ref["tree_bf"]["images"])
    assert not torch.equal(out["match_dist"], ref["match_dist"])
    want = ((lat[:, :, None] - ref["inputs"]["enc_traj_seq"][:, None]) ** 2).mean(-1)
    assert torch.allclose(out["cost_df"], want, rtol=1e-4, atol=1e-6)
    _, total = O.losses(sd, hpl, inputs, out)
    assert torch.isfinite(total)
