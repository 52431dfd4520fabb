"""The loss with the object count on the device (``SymTensors.n_obj`` -> ``catre_loss_fwd3`` / ``catre_loss_bwd3``): a batch
of capacity C whose first n rows are objects gives, bit for bit, what a plain call on those n rows gives - every loss slot,
the 14 logging scalars, the running sums, the gradients - whatever the rows behind hold, and those rows get +0 gradients."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, M = 70, 40
COUNTS = (1, 64, 65, 70)   # 64 / 65: either side of the reduction's 64-lane stride; 70: nothing padded

FORMS = {
    "shipped": {},
    "pm_rt": dict(PM_R_ONLY=False, PM_DISENTANGLE_T=False, PM_DISENTANGLE_Z=False, PM_T_USE_POINTS=True),
    "r_xy_z_points_l2": dict(PM_R_ONLY=False, PM_DISENTANGLE_T=True, PM_DISENTANGLE_Z=True, PM_T_USE_POINTS=True,
                             PM_LOSS_TYPE="L2"),
    "bbox": dict(PM_USE_BBOX=True),
}


def _is_sym(i):
    return i % 3 == 1 or i in (0, 63, 64, 69)   # mixed on both sides of every count


@pytest.fixture(scope="module")
def data():
    """Estimates, ground truth and symmetry info of C objects, and a second set that differs in every row."""
    from catre_amd import synth
    from oracle.aug_oracle import euler2mat
    from oracle.catre_oracle import y_axis_symmetries

    sets = []
    for seed in (41, 42):
        inp = synth.make_inputs(C, 16, M, seed=seed)
        g = torch.Generator().manual_seed(seed)
        rot = (euler2mat(torch.randn(C, 3, generator=g) * 0.3) @ inp["gt_rot"]).contiguous()
        pose = torch.cat([rot, (inp["gt_trans"] + 0.05 * torch.randn(C, 3, generator=g)).unsqueeze(-1)], -1)
        d = dict(pose=pose, scale=inp["gt_scale"] + 0.02 * torch.randn(C, 3, generator=g), gt_rot=inp["gt_rot"],
                 gt_trans=inp["gt_trans"], gt_scale=inp["gt_scale"], kps=inp["obj_kps"],
                 td=0.01 * torch.randn(C, 3, generator=g))
        sets.append({k: v.to(DEV).contiguous() for k, v in d.items()})
    sym12, sym7 = y_axis_symmetries(12), y_axis_symmetries(7)
    sym_a = [(sym12 if i % 2 else sym7) if _is_sym(i) else None for i in range(C)]
    sym_b = [None if _is_sym(i) else sym12 for i in range(C)]   # the other set flips every is_sym
    return sets, (sym_a, sym_b)


def _cfg(form):
    from catre_amd.config import default_cfg

    cfg = default_cfg(num_pcl=16, num_kps=M, device=DEV)
    for k, v in FORMS[form].items():
        cfg.MODEL.CATRE.LOSS_CFG[k] = v
    return cfg


def _run(cfg, d, sym, rows, n_obj=None):
    """catre_loss on the first `rows` rows -> (8 loss slots, 14 scalars, running sums, dpose, dscale)."""
    from catre_amd.losses import SymTensors, catre_loss

    pose = d["pose"][:rows].clone().requires_grad_(True)
    scale = d["scale"][:rows].clone().requires_grad_(True)
    st = SymTensors.from_list(sym[:rows], DEV, s1=13, n_obj=n_obj)
    ld, vis = catre_loss(cfg, pose[:, :3, :3], pose[:, :3, 3], scale, d["gt_rot"][:rows], d["gt_trans"][:rows],
                         d["gt_scale"][:rows], d["kps"][:rows], st, trans_deltas=d["td"][:rows], return_vis=True, pose=pose)
    terms = list(ld.values())
    sums, acc = [], 0
    for t in terms:
        acc = acc + t
        sums.append(acc.detach().clone())
    # distinct upstream gradients for the terms and for the running sum
    (acc + sum((1.0 + 0.25 * i) * t for i, t in enumerate(terms))).backward()
    from catre_amd.losses import loss_block

    return (list(ld), loss_block(vis).clone(), torch.stack(sums), pose.grad.clone(), scale.grad.clone())


@pytest.mark.parametrize("form", list(FORMS))
def test_counted_loss_carries_the_bits_of_a_plain_call_on_the_first_n_rows(form, data):
    (a, b), (sym_a, sym_b) = data
    cfg = _cfg(form)
    for n in COUNTS:
        keys0, block0, sums0, dpose0, dscale0 = _run(cfg, a, sym_a, n)   # the plain entry points on n rows
        keys, block, sums, dpose, dscale = _run(cfg, a, sym_a, C, n_obj=n)
        assert keys == keys0
        assert torch.equal(block, block0), (form, n, (block - block0).abs().max().item())
        assert torch.equal(sums, sums0), (form, n)
        assert tuple(dpose.shape) == (C, 3, 4) and tuple(dscale.shape) == (C, 3)
        assert torch.equal(dpose[:n], dpose0) and torch.equal(dscale[:n], dscale0), (form, n)
        for t in (dpose[n:], dscale[n:]):   # +0.0f, not merely == 0
            assert torch.equal(t.view(torch.int32), torch.zeros_like(t, dtype=torch.int32)), (form, n)
        assert float(block0[0]) > 0 and float(dpose0.abs().max()) > 0   # the comparison is not of zeros

        # other rows behind n (estimates, ground truth, key points, symmetry candidates and flags): not one bit moves
        mixed = {k: torch.cat([a[k][:n], b[k][n:]]) for k in a}
        keys2, block2, sums2, dpose2, dscale2 = _run(cfg, mixed, sym_a[:n] + sym_b[n:], C, n_obj=n)
        assert keys2 == keys0 and torch.equal(block2, block0) and torch.equal(sums2, sums0), (form, n)
        assert torch.equal(dpose2, dpose) and torch.equal(dscale2, dscale), (form, n)


def test_count_is_read_on_the_device_when_the_kernels_run(data):
    """The same tensors, the count rewritten in place between two calls (what a graph replay does)."""
    (a, _), (sym_a, _) = data
    cfg = _cfg("shipped")
    n_obj = torch.tensor([5], dtype=torch.int32, device=DEV)
    got5 = _run(cfg, a, sym_a, C, n_obj=n_obj)
    n_obj.fill_(33)
    got33 = _run(cfg, a, sym_a, C, n_obj=n_obj)
    for n, got in ((5, got5), (33, got33)):
        want = _run(cfg, a, sym_a, n)
        assert torch.equal(got[1], want[1]) and torch.equal(got[3][:n], want[3]) and not got[3][n:].any()


def test_existing_entry_points_do_not_read_a_count(data):
    """Without n_obj the *2 pair runs (B objects, B in every divisor): the C-row result differs from the n-row one."""
    (a, _), (sym_a, _) = data
    cfg = _cfg("shipped")
    full, part = _run(cfg, a, sym_a, C), _run(cfg, a, sym_a, 64)
    assert not torch.equal(full[1], part[1]) and bool(full[3][64:].any())
