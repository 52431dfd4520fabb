"""Every form of the point-matching loss the reference's config can select (PyPMLoss, core/catre/losses/pm_loss.py:21-194):
six structural modes x {l1, smooth_l1, mse, l2} x with-scale x symmetric x bbox points, on the device, against fixtures
written by the unmodified reference (tools/make_pm_loss_golden.py).

Tolerances are those of tests/test_hip_train.py for this kind of comparison: loss values rtol 1e-4 / atol 1e-7 against the
reference's, gradients within 2e-4 of the tensor's largest reference entry.  No case is skipped or filtered."""
import ctypes
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

from catre_amd import hip
from catre_amd.config import default_cfg
from tests.util import GOLDEN_DIR, recipe_sd

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODE_SWITCHES = {   # mode name -> LOSS_CFG switches (PM_T_USE_POINTS spelled out: its default is True)
    "r_only": dict(PM_R_ONLY=True),
    "rt": dict(PM_R_ONLY=False, PM_DISENTANGLE_T=False, PM_DISENTANGLE_Z=False, PM_T_USE_POINTS=True),
    "r_t_points": dict(PM_R_ONLY=False, PM_DISENTANGLE_T=True, PM_DISENTANGLE_Z=False, PM_T_USE_POINTS=True),
    "r_t_direct": dict(PM_R_ONLY=False, PM_DISENTANGLE_T=True, PM_DISENTANGLE_Z=False, PM_T_USE_POINTS=False),
    "r_xy_z_points": dict(PM_R_ONLY=False, PM_DISENTANGLE_T=True, PM_DISENTANGLE_Z=True, PM_T_USE_POINTS=True),
    "r_xy_z_direct": dict(PM_R_ONLY=False, PM_DISENTANGLE_T=True, PM_DISENTANGLE_Z=True, PM_T_USE_POINTS=False),
}
MODE_KEYS = {
    "r_only": ["loss_PM_R"], "rt": ["loss_PM_RT"], "r_t_points": ["loss_PM_R", "loss_PM_T"],
    "r_t_direct": ["loss_PM_R", "loss_PM_T_noP"], "r_xy_z_points": ["loss_PM_R", "loss_PM_xy", "loss_PM_z"],
    "r_xy_z_direct": ["loss_PM_R", "loss_PM_xy_noP", "loss_PM_z_noP"],
}


def _forms():
    z = np.load(os.path.join(GOLDEN_DIR, "pm_loss_forms.npz"), allow_pickle=False)
    return z


def _pm_cfg(mode, elem, with_scale, symmetric, bbox, beta, lw, M, device, others_off=True):
    cfg = default_cfg(num_pcl=64, num_kps=M, device=device)
    lc = cfg.MODEL.CATRE.LOSS_CFG
    for k, v in MODE_SWITCHES[mode].items():
        lc[k] = v
    lc.PM_LOSS_TYPE, lc.PM_SMOOTH_L1_BETA, lc.PM_LW = elem, beta, lw
    lc.PM_WITH_SCALE, lc.PM_LOSS_SYM, lc.PM_USE_BBOX = bool(with_scale), bool(symmetric), bool(bbox)
    if others_off:
        lc.ROT_LW = lc.TRANS_LW = lc.SCALE_LW = 0.0
    return cfg


# ---- 6. host side: the config mapping -------------------------------------------------------------------------------
def test_switch_combinations_map_to_the_mode_the_reference_takes():
    """pm_loss.py:56-68 and the branch order of :126-191, for all 16 combinations of the four switches."""
    from catre_amd.losses import PM_KEYS, PM_MODES, _loss_cfg_struct, pm_mode

    for r_only, dis_t, dis_z, use_pts in itertools.product((False, True), repeat=4):
        cfg = default_cfg(device="cpu")
        lc = cfg.MODEL.CATRE.LOSS_CFG
        lc.PM_R_ONLY, lc.PM_DISENTANGLE_T, lc.PM_DISENTANGLE_Z, lc.PM_T_USE_POINTS = r_only, dis_t, dis_z, use_pts
        # what PyPMLoss.__init__ / forward do with these four
        t, pts = dis_t, use_pts
        if dis_z and not dis_t:
            t = True                      # "disentangle_z means: disentangle R/xy/z"
        if not dis_t and not dis_z:
            pts = True                    # "if not disentangled, must use points to compute t loss"
        if r_only:
            want = "r_only"
        elif dis_z:
            want = "r_xy_z_points" if pts else "r_xy_z_direct"
        elif t:
            want = "r_t_points" if pts else "r_t_direct"
        else:
            want = "rt"
        assert PM_MODES[pm_mode(lc)] == want, (r_only, dis_t, dis_z, use_pts)
        c = _loss_cfg_struct(cfg)
        assert PM_MODES[c.pm_mode] == want and [k for k, _ in PM_KEYS[c.pm_mode]] == MODE_KEYS[want]
    # the two forced cases, spelled out
    cfg = default_cfg(device="cpu")
    lc = cfg.MODEL.CATRE.LOSS_CFG
    lc.PM_R_ONLY, lc.PM_DISENTANGLE_T, lc.PM_DISENTANGLE_Z, lc.PM_T_USE_POINTS = False, False, True, False
    assert PM_MODES[pm_mode(lc)] == "r_xy_z_direct"          # disentangle_z forces disentangle_t
    lc.PM_DISENTANGLE_Z, lc.PM_T_USE_POINTS = False, False
    assert PM_MODES[pm_mode(lc)] == "rt"                      # nothing disentangled: points are used whatever the switch says


def test_element_loss_names_and_the_unknown_one():
    from catre_amd.losses import _loss_cfg_struct

    for name, want in (("L1", 0), ("l1", 0), ("Smooth_L1", 1), ("smooth_l1", 1), ("MSE", 2), ("mse", 2), ("L2", 3), ("l2", 3)):
        cfg = default_cfg(device="cpu")
        cfg.MODEL.CATRE.LOSS_CFG.PM_LOSS_TYPE = name
        cfg.MODEL.CATRE.LOSS_CFG.PM_SMOOTH_L1_BETA = 0.25
        c = _loss_cfg_struct(cfg)
        assert c.pm_elem == want and abs(c.pm_beta - 0.25) < 1e-7
    cfg = default_cfg(device="cpu")
    cfg.MODEL.CATRE.LOSS_CFG.PM_LOSS_TYPE = "huber"
    with pytest.raises(ValueError, match="loss type huber not supported."):   # pm_loss.py:82
        _loss_cfg_struct(cfg)
    cfg.MODEL.CATRE.LOSS_CFG.PM_LW = 0.0    # PM off: PyPMLoss is never constructed (CATRE_disR_shared.py:185)
    assert _loss_cfg_struct(cfg).pm_on == 0
    # the shipped configuration is the R-only / L1 / key-point form, and the struct starts with the old one
    c = _loss_cfg_struct(default_cfg(device="cpu"))
    assert (c.pm_mode, c.pm_elem, c.pm_use_bbox) == (hip.PM_R_ONLY, hip.PM_ELEM_L1, 0)
    assert ctypes.sizeof(hip.CatreLossCfg2) == ctypes.sizeof(hip.CatreLossCfg) + 16 and hip.CatreLossCfg2.base.offset == 0


def test_forms_fixture_is_complete():
    z = _forms()
    cases = z["cases"]
    assert cases.shape == (192, 5) and len({tuple(c) for c in cases.tolist()}) == 192
    assert [str(m) for m in z["meta_modes"]] == list(MODE_SWITCHES) and len(z["meta_elems"]) == 4
    for c, keys in zip(cases.tolist(), z["keys"]):
        assert str(keys).split(",") == MODE_KEYS[str(z["meta_modes"][c[0]])]
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "pm_loss_forms.npz")) < 65463   # smaller than train_b4_t64.npz


# ---- 5. C ABI ----------------------------------------------------------------------------------------------------------
def test_c_program_naming_the_new_symbols_links(tmp_path):
    import shutil
    import subprocess

    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    src = tmp_path / "abi2.c"
    src.write_text(
        '#include <string.h>\n#include <stddef.h>\n#include "catre_hip.h"\n'
        "int main(void) {\n"
        "  catre_loss_cfg2 c; memset(&c, 0, sizeof c);\n"
        "  if (sizeof(catre_loss_cfg2) != sizeof(catre_loss_cfg) + 16 || offsetof(catre_loss_cfg2, base) != 0) return 2;\n"
        "  if (sizeof(catre_loss_cfg) != 60) return 3;\n"
        "  c.pm_mode = CATRE_PM_R_XY_Z_DIRECT; c.pm_elem = CATRE_PM_ELEM_L2;\n"
        "  if (CATRE_PM_MODE_COUNT != 6 || CATRE_PM_ELEM_COUNT != 4 || CATRE_LOSS2_TERMS != 8) return 4;\n"
        "  /* no pointers: refused before any launch */\n"
        "  if (catre_loss_fwd2(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &c, NULL, NULL, NULL, NULL, NULL, NULL, 0,\n"
        "                      NULL, 1, 8, 1, NULL) != CATRE_ERR_BAD_ARG) return 5;\n"
        "  if (catre_loss_bwd2(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, &c, NULL, NULL,\n"
        "                      1, 8, 1, NULL) != CATRE_ERR_BAD_ARG) return 6;\n"
        "  return 0;\n}\n")
    exe = tmp_path / "abi2"
    libdir = os.path.dirname(hip.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe),
                    f"-L{libdir}", "-lcatre_hip", f"-Wl,-rpath,{libdir}"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


BAD_ARG = -1   # CATRE_ERR_BAD_ARG


@pytest.mark.gpu
def test_unknown_mode_or_element_loss_is_refused_without_a_launch():
    lib, st = hip.load(), hip.stream_ptr(torch.device(DEV))
    z, out = torch.zeros(256, device=DEV), torch.zeros(64, device=DEV)
    pz = hip.ptr(z)
    po = hip.ptr(out)
    for mode, elem in ((6, 0), (-1, 0), (0, 4), (0, -1)):
        c = hip.CatreLossCfg2()
        c.pm_on, c.pm_mode, c.pm_elem = 1, mode, elem
        r = lib.catre_loss_fwd2(pz, pz, pz, pz, pz, pz, pz, pz, pz, ctypes.byref(c), po, po, po, po, None, None, 0, None, 2, 8, 1,
                                st)
        assert r == BAD_ARG, (mode, elem, r)
        r = lib.catre_loss_bwd2(pz, pz, pz, pz, pz, pz, pz, pz, pz, pz, pz, None, None, 0, ctypes.byref(c), po, po, 2, 8, 1, st)
        assert r == BAD_ARG, (mode, elem, r)
    # nine terms, a term index of 8; bbox points with M != 8
    c = hip.CatreLossCfg2()
    c.pm_on = 1
    terms = (ctypes.c_int32 * 9)(*range(8), 0)
    assert lib.catre_loss_fwd2(pz, pz, pz, pz, pz, pz, pz, pz, pz, ctypes.byref(c), po, po, po, po, None, terms, 9, po, 2, 8, 1,
                               st) == BAD_ARG
    bad = (ctypes.c_int32 * 1)(8)
    assert lib.catre_loss_fwd2(pz, pz, pz, pz, pz, pz, pz, pz, pz, ctypes.byref(c), po, po, po, po, None, bad, 1, po, 2, 8, 1,
                               st) == BAD_ARG
    c.pm_use_bbox = 1
    assert lib.catre_loss_fwd2(pz, pz, pz, pz, pz, None, pz, pz, pz, ctypes.byref(c), po, po, po, po, None, None, 0, None, 2, 9, 1,
                               st) == BAD_ARG
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(z.abs().max()) == 0.0


# ---- 1. every form against the reference ----------------------------------------------------------------------------
def _case_id(c):
    return "-".join(str(x) for x in c)


_CASES = [tuple(int(v) for v in c) for c in _forms()["cases"].tolist()]


@pytest.mark.gpu
@pytest.mark.parametrize("case", _CASES, ids=_case_id)
def test_every_form_matches_the_reference(case):
    """catre_loss with the matching LOSS_CFG (other terms off): the reference's keys in its order, its values, and after
    sum(ld.values()).backward() its gradients of rotation, translation and scale."""
    from catre_amd.losses import catre_loss
    from oracle.catre_oracle import y_axis_symmetries

    z = _forms()
    idx = _CASES.index(case)
    mi, ei, ws, symmetric, bbox = case
    mode, elem = str(z["meta_modes"][mi]), str(z["meta_elems"][ei])
    B, M, _ = (int(v) for v in z["meta"])
    beta, lw = (float(v) for v in z["meta_beta_lw"])
    cfg = _pm_cfg(mode, elem, ws, symmetric, bbox, beta, lw, M, DEV)
    sym = [None if n == 0 else y_axis_symmetries(int(n) + 1) for n in z["meta_nsym"]]
    t = lambda k: torch.from_numpy(z[f"in_{k}"]).to(DEV)
    r, tr, s = (t(k).clone().requires_grad_(True) for k in ("pred_rots", "pred_transes", "pred_scales"))
    ld = catre_loss(cfg, r, tr, s, t("gt_rots"), t("gt_transes"), t("gt_scales"), t("points"), sym)
    want_keys = str(z["keys"][idx]).split(",")
    assert list(ld) == want_keys
    sum(ld.values()).backward()
    got = {k: v.item() for k, v in ld.items()}
    grads = {}
    for name, leaf, ref in (("rot", r, z["grad_rot"][idx]), ("trans", tr, z["grad_trans"][idx]), ("scale", s, z["grad_scale"][idx])):
        g = leaf.grad.cpu().numpy() if leaf.grad is not None else np.zeros_like(ref)
        top = float(np.abs(ref).max())
        grads[name] = (float(np.abs(g - ref).max()), top)
    print(f"case {mode}/{elem}/scale={ws}/sym={symmetric}/bbox={bbox}: " +
          ", ".join(f"{k} {got[k]:.7g} (ref {z['vals'][idx][j]:.7g})" for j, k in enumerate(want_keys)) + "; " +
          ", ".join(f"d{k} err {e:.2e} of max {m:.2e}" for k, (e, m) in grads.items()))
    for j, k in enumerate(want_keys):
        np.testing.assert_allclose(got[k], z["vals"][idx][j], rtol=1e-4, atol=1e-7, err_msg=k)
    for name, (err, top) in grads.items():
        assert err <= 2e-4 * top + 1e-12, (name, err, top)
    # gradients reach t in every non-R-only form and the scale exactly when with_scale is on
    assert (grads["trans"][1] > 0) == (mode != "r_only") and (grads["scale"][1] > 0) == bool(ws)


# ---- 2. whole iteration ---------------------------------------------------------------------------------------------------
def _load_train_golden_with_overrides(name):
    import ast

    from tests.util import load_train_golden

    g = load_train_golden(name)
    z = np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"), allow_pickle=False)
    for path, v in ast.literal_eval(str(z["meta_overrides"])):
        node = g["cfg"]
        keys = path.split(".")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = v
    g["loss_keys"] = str(z["meta_loss_keys"]).split(",")
    return g


@pytest.mark.gpu
def test_training_iteration_with_the_base_configs_pm_defaults():
    """model(..., do_loss=True) with PM_R_ONLY=False (configs/_base_/catre_base.py:233-244): loss_PM_RT in front of the five
    other terms, refined pose, gradient norms and heads against the reference's own iteration - the bounds of
    test_hip_train.test_module_training_step_matches_reference_golden."""
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer

    g = _load_train_golden_with_overrides("train_b4_t64_pm_rt")
    cfg = g["cfg"].__deepcopy__({})
    assert cfg.MODEL.CATRE.LOSS_CFG.PM_R_ONLY is False
    cfg.MODEL.DEVICE = DEV
    model, _ = build_model_optimizer(cfg, is_test=False)
    model.load_state_dict({k: v.to(DEV) for k, v in recipe_sd(cfg, g["salt"]).items()}, strict=True)
    model.train()
    b = {k: v.to(DEV) for k, v in g["batch"].items()}
    batch_updater_test(cfg, b)
    out_dict, loss_dict = model(
        b["x"], b["tfd_kps"], init_pose=b["obj_pose_est"], init_scale=b["obj_scale_est"], K_zoom=b["K"],
        obj_class=b["obj_cls"], gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"], gt_scale=b["gt_scale"],
        obj_kps=b["obj_kps"], mean_scales=b["obj_mean_scales"], sym_info=g["sym_info"], do_loss=True, cur_iter=1)
    ref = g["ref"]
    assert np.abs(out_dict["pose_1"].detach().cpu().numpy() - ref["pose_1"]).max() <= 2e-5
    assert np.abs(out_dict["scale_1"].detach().cpu().numpy() - ref["scale_1"]).max() <= 2e-5
    assert list(loss_dict) == g["loss_keys"] and g["loss_keys"][0] == "loss_PM_RT" and len(loss_dict) == 6
    for k, v in loss_dict.items():
        print(f"{k}: {v.item():.7g} (ref {float(ref[f'loss__{k}'][0]):.7g})")
        np.testing.assert_allclose(v.item(), ref[f"loss__{k}"][0], rtol=1e-4, atol=1e-7, err_msg=k)
    sum(loss_dict.values()).backward()
    for k, p in model.named_parameters():
        if f"gradnone__{k}" in ref:
            assert p.grad is None, k
            continue
        nrm = float(ref[f"gradnorm__{k}"][0])
        got = p.grad.cpu()
        np.testing.assert_allclose(float(got.norm()), nrm, rtol=1e-3, atol=1e-9, err_msg=k)
        np.testing.assert_allclose(got.reshape(-1)[:64].numpy(), ref[f"gradhead__{k}"], atol=1e-3 * nrm + 1e-9, rtol=0,
                                   err_msg=k)
    vis = model.vis_scalars.as_dict()
    want = {k[5:].replace("__", "/"): float(v[0]) for k, v in ref.items() if k.startswith("vis__")}
    assert set(vis) == set(want) and len(vis) == 14
    for k in want:
        np.testing.assert_allclose(vis[k], want[k], rtol=2e-4, atol=2e-5, err_msg=k)


# ---- 3. nothing moved ---------------------------------------------------------------------------------------------------
def _abi_record():
    spec = importlib.util.spec_from_file_location("loss_abi_record", os.path.join(ROOT, "profiles", "loss_abi_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_old_entry_points_keep_the_bits_of_the_previous_library():
    """tests/golden/loss_abi_shipped.npz was written by profiles/loss_abi_record.py with the library of the commit before
    the other PM forms existed (`train_b4` inputs, shipped configuration): catre_loss_{fwd,bwd}{,_sums} still return
    those bits - losses[20], best, counts, prefix, dpose, dscale."""
    rec = _abi_record()
    got = rec.run_old_entry_points(DEV)
    want = dict(np.load(os.path.join(GOLDEN_DIR, "loss_abi_shipped.npz")))
    assert set(got) == set(want) and len(want) == 11
    assert rec.compare(got, want) == []


@pytest.mark.gpu
def test_new_entry_points_return_the_old_ones_bits_for_the_shipped_form():
    """catre_loss_fwd2 / catre_loss_bwd2 with (R only, l1, key points): slots 0..5, the 14 scalars, the running sums, dpose
    and dscale bit-identical to catre_loss_fwd_sums / catre_loss_bwd_sums on the `train_b4` inputs; slots 6, 7 are 0."""
    rec = _abi_record()
    old = rec.run_old_entry_points(DEV)
    lib, p = hip.load(), hip.ptr
    x = rec.shipped_inputs(DEV)
    from catre_amd.losses import _loss_cfg_struct

    c = _loss_cfg_struct(x["cfg"])
    B, M, S1 = x["B"], x["M"], x["cands"].shape[1]
    st = hip.stream_ptr(torch.device(DEV))
    best = torch.empty(B, dtype=torch.int32, device=DEV)
    counts = torch.empty(2, dtype=torch.int32, device=DEV)
    part = torch.empty(B * hip.LOSS2_PART, device=DEV)
    losses, prefix = torch.full((22,), 7.0, device=DEV), torch.zeros(6, device=DEV)
    terms = (ctypes.c_int32 * 6)(*rec.TERMS)
    head = (p(x["pose"]), p(x["scale"]), p(x["gt_rot"]), p(x["gt_trans"]), p(x["gt_scale"]), p(x["kps"]), p(x["cands"]))
    hip.check(lib.catre_loss_fwd2(*head, p(x["valid"]), p(x["is_sym"]), ctypes.byref(c), p(best), p(counts), p(part), p(losses),
                                  None, terms, 6, p(prefix), B, M, S1, st), "catre_loss_fwd2")
    up = torch.tensor(rec.UPSTREAM + (3.0, 5.0), device=DEV)     # slots 6, 7 do not exist in this form: ignored
    ups = [torch.full((1,), 0.125 * (k + 1), device=DEV) for k in range(6)]
    parr = (ctypes.c_void_p * 6)(*[u.data_ptr() for u in ups])
    dpose, dscale = torch.zeros(B, 3, 4, device=DEV), torch.zeros(B, 3, device=DEV)
    hip.check(lib.catre_loss_bwd2(*head, p(x["is_sym"]), p(best), p(counts), p(up), parr, terms, 6, ctypes.byref(c), p(dpose),
                                  p(dscale), B, M, S1, st), "catre_loss_bwd2")
    torch.cuda.synchronize()
    bits = lambda t: t.cpu().contiguous().view(torch.int32).numpy()
    assert np.array_equal(bits(losses[:6]), old["sums_losses"][:6]) and np.array_equal(bits(losses[8:]), old["sums_losses"][6:])
    assert float(losses[6]) == 0.0 and float(losses[7]) == 0.0
    assert np.array_equal(bits(prefix), old["sums_prefix"])
    assert np.array_equal(best.cpu().numpy(), old["sums_best"]) and np.array_equal(counts.cpu().numpy(), old["sums_counts"])
    assert np.array_equal(bits(dpose), old["sums_dpose"]) and np.array_equal(bits(dscale), old["sums_dscale"])


# ---- 4. chain and graph ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["r_xy_z_points", "r_xy_z_direct"])
def test_eight_term_dict_sums_along_the_precomputed_chain(mode, monkeypatch):
    """A three-term PM form with every other loss on: eight dict entries.  sum(ld.values()) is the running sum the kernel
    wrote - the bits of the same chain as plain torch adds - with one loss-backward launch and no add node."""
    from catre_amd import synth
    from catre_amd.losses import _LossTerm, catre_loss
    from oracle import catre_oracle as O
    from oracle.aug_oracle import euler2mat

    B, M = 9, 96
    cfg = _pm_cfg(mode, "Smooth_L1", 1, 1, 0, 0.05, 1.5, M, DEV, others_off=False)
    inp = synth.make_inputs(B, 64, M, seed=31)
    g = torch.Generator().manual_seed(5)
    sym = [O.y_axis_symmetries(12) if i in (0, 3) else None for i in range(B)]
    out_rot = (euler2mat(torch.randn(B, 3, generator=g) * 0.2) @ inp["gt_rot"]).contiguous()
    out_trans = inp["gt_trans"] + 0.05 * torch.randn(B, 3, generator=g)
    out_scale = inp["gt_scale"] + 0.02 * torch.randn(B, 3, generator=g)
    dv = lambda x: x.to(DEV)
    lib = hip.load()
    calls = []
    orig = lib.catre_loss_bwd2

    def counting(*a):
        calls.append(1)
        return orig(*a)

    monkeypatch.setattr(lib, "catre_loss_bwd2", counting)

    def run(total_of):
        r, t, s = (x.clone().to(DEV).requires_grad_(True) for x in (out_rot, out_trans, out_scale))
        ld = catre_loss(cfg, r, t, s, dv(inp["gt_rot"]), dv(inp["gt_trans"]), dv(inp["gt_scale"]), dv(inp["obj_kps"]), sym)
        tot = total_of(ld)
        n0 = len(calls)
        tot.backward()
        return ld, tot, [x.grad.clone() for x in (r, t, s)], len(calls) - n0

    def plain_chain(ld):
        acc = 0
        for v in ld.values():
            acc = acc + v.as_subclass(torch.Tensor)
        return acc

    ld, tot, grads, n_bwd = run(lambda ld: sum(ld.values()))
    ld2, tot2, grads2, n_bwd2 = run(plain_chain)
    assert list(ld) == MODE_KEYS[mode] + ["loss_rot", "loss_yaxis_rot", "loss_trans_xy", "loss_trans_z", "loss_scale"]
    assert len(ld) == 8 and all(v.item() > 0 for v in ld.values())
    assert isinstance(tot, _LossTerm) and type(tot2) is torch.Tensor
    assert tot.grad_fn is not None and "Add" not in type(tot.grad_fn).__name__      # no add kernel ran
    assert n_bwd == 1 and n_bwd2 == 1                                               # one loss-backward launch
    assert torch.equal(tot.detach().as_subclass(torch.Tensor), tot2.detach())
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)
    # python's sum() over the plain values, on the host in fp32: the same bits once more
    acc = np.float32(0)
    for v in ld2.values():
        acc = np.float32(acc + np.float32(v.item()))
    assert np.float32(tot.item()).tobytes() == acc.tobytes()


@pytest.mark.gpu
def test_graphed_train_step_replays_a_three_term_form():
    """GraphedTrainStep captures and replays a step with the R / xy / z point form (eight loss terms): losses, refined pose
    and every parameter after each step equal the eager loop's, bit for bit."""
    from catre_amd import synth
    from catre_amd.batching import batch_updater_test
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.graphed import GraphedTrainStep
    from oracle.catre_oracle import y_axis_symmetries

    B, N, M = 6, 128, 64
    cfg = default_cfg(num_pcl=N, num_kps=M, device=DEV)
    lc = cfg.MODEL.CATRE.LOSS_CFG
    for k, v in MODE_SWITCHES["r_xy_z_points"].items():
        lc[k] = v
    lc.PM_LOSS_TYPE, lc.PM_SMOOTH_L1_BETA = "L2", 0.05
    sd = {k: v.to(DEV) for k, v in synth.recipe_state_dict(expected_state_shapes(cfg)).items()}
    sym12, sym7 = y_axis_symmetries(12), y_axis_symmetries(7)
    batches, syms = [], []
    for i in range(3):
        b = {k: v.to(DEV) for k, v in synth.make_inputs(B, N, M, seed=60 + i).items()}
        batch_updater_test(cfg, b)
        batches.append(b)
        syms.append([(sym12 if (j + i) % 3 == 0 else (sym7 if (j * i) % 4 == 1 else None)) for j in range(B)])

    def kwargs(b):
        return dict(x=b["x"].contiguous(), tfd_kps=b["tfd_kps"].contiguous(), init_pose=b["obj_pose_est"],
                    init_scale=b["obj_scale_est"], K_zoom=b["K"], gt_ego_rot=b["gt_rot"], gt_trans=b["gt_trans"],
                    gt_scale=b["gt_scale"], obj_kps=b["obj_kps"], mean_scales=b["obj_mean_scales"])

    model_e, opt_e = build_model_optimizer(cfg, is_test=False)
    model_e.load_state_dict(sd)
    eager = []
    for b, s in zip(batches, syms):
        kw = kwargs(b)
        out, ld = model_e(kw.pop("x"), kw.pop("tfd_kps"), sym_info=s, do_loss=True, cur_iter=1, **kw)
        sum(ld.values()).backward()
        opt_e.step()
        opt_e.zero_grad(set_to_none=True)
        eager.append(({k: v.detach().as_subclass(torch.Tensor).clone() for k, v in ld.items()}, out["pose_1"].detach().clone(),
                      {k: p.detach().clone() for k, p in model_e.named_parameters()}))
    assert list(eager[0][0]) == MODE_KEYS["r_xy_z_points"] + ["loss_rot", "loss_yaxis_rot", "loss_trans_xy", "loss_trans_z",
                                                              "loss_scale"]

    model_g, opt_g = build_model_optimizer(cfg, is_test=False)
    model_g.load_state_dict(sd)
    step = GraphedTrainStep(model_g, opt_g, kwargs(batches[0]), syms[0], max_sym=12)
    for i, (b, s) in enumerate(zip(batches, syms)):
        out, ld = step(sym_info=s, **kwargs(b))
        torch.cuda.synchronize()
        want_l, want_pose, want_p = eager[i]
        assert list(ld) == list(want_l)
        for k, v in want_l.items():
            assert torch.equal(ld[k].detach().as_subclass(torch.Tensor).reshape(()), v.reshape(())), f"step {i} {k}"
        assert torch.equal(out["pose_1"], want_pose), f"step {i}: pose"
        for k, p in model_g.named_parameters():
            assert torch.equal(p, want_p[k]), f"step {i}: parameter {k}"
