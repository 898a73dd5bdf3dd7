"""CPU: the premises of the mesh / inertia / world tests of tests/test_igr_shapenet_gpu.py, recomputed on the numpy
restatement (tests/igr_seed_choice.py), and the shapenet plumbing of the inertia driver."""
import numpy as np
import pytest

import igr_seed_choice as SC
import implicit_net as IN


def test_chosen_seed_makes_the_meshsdf_rule_comparable_with_central_differences():
    """For the GPU tests' seed and latent, MeshSDF's rule and the true shape derivative agree within 3.5 % in every component
    of both losses (the GPU tests allow 5 % against central differences), and every component of d trace(J) / d latent is
    far above the 1e-3 below which the tolerance's absolute floor would carry the check.  Seed 0 shows what the choice
    avoids: there the rule is off by four times the tolerance whatever the kernels do."""
    import test_igr_shapenet_gpu as T
    assert (T.SEED, T.RADIUS, tuple(T.LATENT)) == (126, 0.6, SC.LATENT)
    res = SC.rule_vs_true(T.SEED)
    print({k: (np.round(t, 4), np.round(r, 4)) for k, (t, r) in res.items()}, SC.disagreement(res))
    assert SC.disagreement(res) < 0.035
    assert np.abs(res["trace"][0]).min() > 0.05 and np.abs(res["spin"][0]).min() > 0.05
    assert SC.disagreement(SC.rule_vs_true(0)) > 0.2


def test_geometric_init_weights_shapenet():
    """scenes.geometric_init_weights(width=256, latent=4), what `experiments inertia --net shapenet` packs: the shapenet layer
    shapes, the same seeded draw as the tests' restatement, accepted by pack_weights; the default call is unchanged."""
    from diffsdfsim_amd import igr, scenes
    Ws, bs = scenes.geometric_init_weights(3, 0.5, 256, 4)
    assert [w.shape for w in Ws] == igr.layer_shapes(256, 4) == IN.layer_dims(**IN.SHAPENET)
    Wr, br = IN.geometric_init(seed=3, radius_init=0.5, **IN.SHAPENET)
    assert all(np.array_equal(a, b) for a, b in zip(Ws, Wr)) and all(np.array_equal(a, b) for a, b in zip(bs, br))
    assert igr.packed_shape(igr.pack_weights(Ws, bs, device="cpu")) == (256, 4) == igr.SHAPES[1]
    W0, b0 = scenes.geometric_init_weights(3, 0.5)
    Wr, br = IN.geometric_init(seed=3, radius_init=0.5, **IN.BOB_SPOT)
    assert all(np.array_equal(a, b) for a, b in zip(W0, Wr)) and all(np.array_equal(a, b) for a, b in zip(b0, br))


def test_inertia_driver_knows_the_network_names():
    from diffsdfsim_amd import experiments
    with pytest.raises(SystemExit):
        experiments.main(["inertia", "--net", "resnet"])
