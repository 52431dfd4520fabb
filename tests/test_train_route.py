"""The route `train_route` returns is the route `forward_train` builds: after one forward the custom autograd nodes behind
`pose` are the ones a small table maps the TrainRoute to.  Forward only; B = 2, N = M = 64 (one tile per cloud, two clouds per
object), one case at N = 128."""
import pytest
import torch

DEV = "cuda:0"

# the nodes whose presence the route decides
ROUTED = {"_PooledChain", "_PointfeatHub", "_LinearMaxPool", "_MaxPool", "_ObjectMajor", "_RotHeads", "_RotHeadPairLP", "_RotHeadLP",
          "_RotL0Block", "_RotL1Block", "_RotL1TailLP", "_NeckTail", "_RotLinear", "_GNPointsGelu", "_WSum"}


def nodes_of(route):
    """TrainRoute -> the ROUTED nodes its graph holds."""
    enc, want = route.enc, set()
    if enc.kind == "fused":
        want |= {"_PooledChain"} if "chain" in (enc.stn, enc.fstn) else set()
        want |= {"_LinearMaxPool"} if "layered" in (enc.stn, enc.fstn, enc.trunk) else set()
        want |= {"_PointfeatHub"} if enc.trunk == "hub" else {"_MaxPool", "_ObjectMajor"}
    elif enc.kind == "layered":
        want |= {"_LinearMaxPool", "_MaxPool", "_ObjectMajor"}
    first = {"l0_block": {"_RotL0Block"}, "layered": {"_RotLinear", "_GNPointsGelu"}, "lp_node": {"_RotHeadLP"}}
    second = {"l1_block": {"_RotL1Block", "_WSum"}, "l1_tail_lp": {"_RotL1TailLP"}, "neck_tail": {"_RotLinear", "_NeckTail"},
              "layered": {"_RotLinear", "_GNPointsGelu", "_WSum"}, "": set()}
    if route.heads == "fused_f32":
        want |= {"_RotHeads"}
    elif route.heads == "lp_pair":
        want |= {"_RotHeadPairLP"}
    elif route.heads == "split":
        want |= first["l0_block" if route.split[0] else "layered"] | second["l1_tail_lp" if route.split[1] else "neck_tail"]
    elif route.heads == "per_head":
        for h in route.per_head:
            want |= first[h.first] | second[h.second]
    return want


def graph_nodes(t):
    seen, names, todo = set(), set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__.replace("Backward", ""))
        todo += [f for f, _ in fn.next_functions]
    return names


CASES = {
    # name: (amp_mode, autocast, knob overrides, frozen encoder, N), and what the issue names of the expected graph
    "fp32": (None, False, {}, False, 64, {"_RotHeads", "_PointfeatHub", "_PooledChain"}),
    "fp32_n128": (None, False, {}, False, 128, {"_RotHeads", "_PointfeatHub", "_PooledChain"}),
    "autocast": (None, True, {}, False, 64, {"_RotHeadPairLP", "_PointfeatHub"}),
    "split": ("split", False, {}, False, 64, {"_RotL0Block", "_RotL1TailLP"}),
    "autocast_unfused_rot": (None, True, dict(fused_lp_rot=False), False, 64, {"_RotLinear", "_NeckTail"}),
    "split_layerwise": ("split", False, dict(split_l0_one_pass=False, split_l1_one_pass=False), False, 64,
                        {"_RotLinear", "_GNPointsGelu", "_NeckTail"}),
    "fp32_frozen": (None, False, {}, True, 64, {"_RotHeads"}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_route_returned_is_the_route_built(case, monkeypatch):
    from catre_amd import synth, train_forward as TF
    from catre_amd import train_ops as T
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    mode, autocast, knobs, frozen, N, named = CASES[case]
    B, M = 2, 64
    cfg = default_cfg(num_pcl=N, num_kps=M, device=DEV)
    model, _ = build_model_optimizer(cfg, is_test=False)
    model.load_state_dict({k: v.to(DEV) for k, v in synth.recipe_state_dict(expected_state_shapes(cfg)).items()})
    model.train()
    if frozen:
        for q in model.pcl_net.parameters():
            q.requires_grad = False
    b = {k: v.to(DEV) for k, v in synth.make_inputs(B, N, M, seed=23).items()}
    batch_updater_test(cfg, b)
    routes = []
    route_fn = TF.TR.train_route
    monkeypatch.setattr(TF.TR, "train_route", lambda *a: routes.append(route_fn(*a)) or routes[-1])
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast), T.amp_mode(mode), T.train_kernels(knobs):
        pose, scale, _ = TF.forward_train(dict(model.named_parameters()), model._opts, b["x"], b["tfd_kps"], b["obj_pose_est"],
                                          b["obj_scale_est"], b["K"], b["obj_mean_scales"], rt=model._runtime())
    assert len(routes) == 1 and torch.isfinite(pose).all()
    got = graph_nodes(pose) & ROUTED
    print(case, routes[0], sorted(got))
    assert got == nodes_of(routes[0]), (routes[0], sorted(got))
    assert named <= got
    if frozen:
        assert routes[0].enc.kind == "frozen"
