"""Host side of the graphed refine loop: bucket selection, argument validation, the ``n_obj`` member of ``SymTensors`` and
the two entry points behind it.  Nothing here needs a device."""
import os
import re

import numpy as np
import pytest
import torch

from catre_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucket_selection_at_the_edges():
    from catre_amd.graphed import DEFAULT_BUCKETS, pick_bucket

    assert DEFAULT_BUCKETS == (16, 32, 48, 64, 96, 128)
    for n, want in ((1, 16), (16, 16), (17, 32), (64, 64), (65, 96), (110, 128), (128, 128), (129, None), (1000, None)):
        assert pick_bucket(n, DEFAULT_BUCKETS) == want, n
    assert pick_bucket(8, (8,)) == 8 and pick_bucket(9, (8,)) is None


def _model_and_optimizer():
    from catre_amd.CATRE_disR_shared import build_model_optimizer
    from catre_amd.config import default_cfg

    return build_model_optimizer(default_cfg(num_pcl=16, num_kps=8, device="cpu"), is_test=False)


def test_loop_arguments_are_validated():
    from catre_amd.graphed import GraphedTrainLoop

    model, opt = _model_and_optimizer()
    loop = GraphedTrainLoop(model, opt, 16, 8, buckets=(32, 8, 16, 8), max_graphs=2, max_sym=12)
    assert loop.buckets == (8, 16, 32)   # ascending, no duplicates
    assert [loop.bucket_for(n) for n in (8, 9, 32, 33)] == [8, 16, 32, None]
    assert loop.stats() == {} and loop.captures == 0   # nothing is captured before a batch asks for it
    with pytest.raises(TypeError):
        GraphedTrainLoop(model, torch.optim.SGD(model.parameters(), lr=0.1), 16, 8)
    for kw in (dict(buckets=()), dict(buckets=(0, 8)), dict(buckets=(8.5,)), dict(max_graphs=0), dict(max_sym=-1),
               dict(warmup=0)):
        with pytest.raises(ValueError):
            GraphedTrainLoop(model, opt, 16, 8, **kw)
    with pytest.raises(ValueError):
        GraphedTrainLoop(model, opt, 0, 8)

    z = torch.zeros
    batch = dict(pcl=z(3, 16, 3), obj_kps=z(3, 8, 3), obj_pose_est=z(3, 3, 4), obj_scale_est=z(3, 3), gt_rot=z(3, 3, 3),
                 gt_trans=z(3, 3), gt_scale=z(3, 3))
    with pytest.raises(ValueError):
        loop(batch, 0)                                        # n_iter
    with pytest.raises(ValueError):
        loop(batch, 2, sym_info=[None] * 4)                   # one entry per object
    with pytest.raises(ValueError):
        loop(dict(batch, pcl=z(3, 17, 3)), 2)                 # another N than the loop was built for
    with pytest.raises(ValueError):
        loop({k: v[:0] for k, v in batch.items()}, 2)         # no objects
    with pytest.raises(KeyError):
        loop({k: v for k, v in batch.items() if k != "obj_pose_est"}, 2)
    with pytest.raises(KeyError):
        loop({k: v for k, v in batch.items() if k != "gt_rot"}, 2)


def test_loop_rows_takes_the_reference_batch_or_the_synthetic_one():
    from catre_amd.graphed import loop_rows

    z = torch.zeros
    pose = torch.arange(24.0).view(2, 3, 4)
    ref = dict(pcl=z(2, 4, 3), obj_kps=z(2, 4, 3), obj_pose_est=z(2, 3, 4), obj_scale_est=z(2, 3), obj_pose=pose,
               obj_scale=torch.ones(2, 3), K=z(2, 3, 3))
    rows = loop_rows(ref)
    assert torch.equal(rows["gt_rot"], pose[:, :3, :3]) and torch.equal(rows["gt_trans"], pose[:, :3, 3])
    assert torch.equal(rows["gt_scale"], torch.ones(2, 3)) and "obj_mean_scales" not in rows and "K" in rows


def test_heads_of_another_form_are_refused():
    from catre_amd.graphed import GraphedTrainLoop

    model, opt = _model_and_optimizer()
    model._head_forms = lambda: ("something else", "something else")
    with pytest.raises(NotImplementedError):
        GraphedTrainLoop(model, opt, 16, 8)


def test_sym_tensors_carry_an_object_count():
    from catre_amd.losses import SymTensors

    sym = [None, np.stack([np.eye(3, dtype=np.float32)] * 3), None, None]
    plain = SymTensors.from_list(sym, "cpu", s1=6)
    assert plain.n_obj is None
    st = SymTensors.from_list(sym, "cpu", s1=6, n_obj=3)
    assert tuple(st.cands.shape) == (4, 6, 3, 3) and tuple(st.valid.shape) == (4, 6) and tuple(st.is_sym.shape) == (4,)
    assert st.cands.dtype == torch.float32 and st.valid.dtype == torch.uint8 and st.is_sym.dtype == torch.int32
    assert st.n_obj.dtype == torch.int32 and tuple(st.n_obj.shape) == (1,) and int(st.n_obj) == 3
    own = torch.tensor([2], dtype=torch.int32)
    assert SymTensors.from_list(sym, "cpu", n_obj=own).n_obj is own      # a caller's static tensor is taken as it is
    assert SymTensors(st.cands, st.valid, st.is_sym).n_obj is None
    for bad in (0, 5):
        with pytest.raises(ValueError):
            SymTensors.from_list(sym, "cpu", n_obj=bad)
    for bad in (torch.tensor([2]), torch.tensor([1, 2], dtype=torch.int32), 2):
        with pytest.raises(TypeError):
            SymTensors(st.cands, st.valid, st.is_sym, bad)


def test_counted_loss_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "catre_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, like in (("catre_loss_fwd3", "catre_loss_fwd2"), ("catre_loss_bwd3", "catre_loss_bwd2")):
        assert name in hip.EXPORTED_SYMBOLS
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/catre_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        old = [a.strip() for a in re.search(r"\bint\s+" + like + r"\s*\(([^)]*)\)\s*;", src).group(1).split(",")]
        # the arguments of the *2 entry point, then the device count in front of the stream
        assert args == old[:-1] + ["const int32_t* n_obj", "void* stream"], name
        assert len(hip._SIGS[name][1]) == len(hip._SIGS[like][1]) + 1
