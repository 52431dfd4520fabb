"""Record / compare the raw results of the four ``catre_loss_{fwd,bwd}{,_sums}`` entry points for the shipped loss
configuration on the inputs of ``tests/golden/train_b4.npz`` (estimate = the fixture's initial pose / scale).

    python profiles/loss_abi_record.py --write tests/golden/loss_abi_shipped.npz   # on the commit to pin
    python profiles/loss_abi_record.py --check tests/golden/loss_abi_shipped.npz   # on a later commit: every bit equal

The committed file was written by the library of the commit BEFORE the point-matching loss got its other forms, so
``tests/test_pm_loss_forms.py::test_old_entry_points_keep_the_bits_of_the_previous_library`` pins the C ABI's results
to what C callers got then.  Everything is compared as int32 bit patterns, not as floats.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

UPSTREAM = (1.0, 0.75, 1.25, 0.5, 1.5, 2.0)   # distinct per term, so a swapped term shows
TERMS = (0, 1, 2, 3, 4, 5)


def shipped_inputs(dev):
    """-> dict of device tensors: the `train_b4` batch with the initial estimate as the pose the loss sees."""
    from catre_amd.losses import _sym_tensor
    from tests.util import load_train_golden

    g = load_train_golden("train_b4")
    b = g["batch"]
    cands, valid, is_sym = _sym_tensor(list(g["sym_info"]), dev, torch.float32)
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    return dict(cfg=g["cfg"], B=g["B"], M=g["M"], pose=f(b["obj_pose_est"]), scale=f(b["obj_scale_est"]), gt_rot=f(b["gt_rot"]),
                gt_trans=f(b["gt_trans"]), gt_scale=f(b["gt_scale"]), kps=f(b["obj_kps"]), cands=cands.contiguous(),
                valid=valid.contiguous(), is_sym=is_sym.contiguous())


def old_cfg_struct(cfg):
    """The 15-field ``catre_loss_cfg`` of the header, filled for the shipped configuration, laid out by hand (so this
    script does not depend on how catre_amd.hip spells the struct)."""
    class Cfg(ctypes.Structure):
        _fields_ = [(f"i{k}", ctypes.c_int32) for k in range(11)] + [(f"f{k}", ctypes.c_float) for k in range(4)]

    lc = cfg.MODEL.CATRE.LOSS_CFG
    assert lc.PM_LOSS_TYPE == "L1" and lc.PM_R_ONLY and lc.ROT_LOSS_TYPE == "angular" and lc.ROT_YAXIS_LOSS_TYPE == "L1"
    assert lc.TRANS_LOSS_TYPE == "L1" and lc.SCALE_LOSS_TYPE == "L1" and lc.TRANS_LOSS_DISENTANGLE
    return Cfg(1, int(lc.PM_LOSS_SYM), int(lc.PM_WITH_SCALE), 1, 0, 0, 1, 0, 1, 1, 0, lc.PM_LW, lc.ROT_LW, lc.TRANS_LW, lc.SCALE_LW)


def run_old_entry_points(dev="cuda:0"):
    """-> {name: int32 array of the bit patterns}"""
    from catre_amd import hip

    lib, p = hip.load(), hip.ptr
    x = shipped_inputs(dev)
    c = old_cfg_struct(x["cfg"])
    B, M, S1 = x["B"], x["M"], x["cands"].shape[1]
    st = hip.stream_ptr(torch.device(dev))
    out = {}

    def bits(t):
        return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()

    for sums in (False, True):
        tag = "sums" if sums else "plain"
        best = torch.empty(B, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        part = torch.empty(B * 8, dtype=torch.float32, device=dev)
        losses = torch.zeros(20, dtype=torch.float32, device=dev)
        prefix = torch.zeros(6, dtype=torch.float32, device=dev)
        head = (p(x["pose"]), p(x["scale"]), p(x["gt_rot"]), p(x["gt_trans"]), p(x["gt_scale"]), p(x["kps"]), p(x["cands"]))
        if sums:
            terms = (ctypes.c_int32 * 6)(*TERMS)
            hip.check(lib.catre_loss_fwd_sums(*head, p(x["valid"]), p(x["is_sym"]), ctypes.byref(c), p(best), p(counts), p(part),
                                              p(losses), None, terms, 6, p(prefix), B, M, S1, st), "catre_loss_fwd_sums")
        else:
            hip.check(lib.catre_loss_fwd(*head, p(x["valid"]), p(x["is_sym"]), ctypes.byref(c), p(best), p(counts), p(part),
                                         p(losses), None, B, M, S1, st), "catre_loss_fwd")
        up = torch.tensor(UPSTREAM, dtype=torch.float32, device=dev)
        dpose, dscale = torch.zeros(B, 3, 4, device=dev), torch.zeros(B, 3, device=dev)
        if sums:
            ups = [torch.full((1,), 0.125 * (k + 1), device=dev) for k in range(6)]
            parr = (ctypes.c_void_p * 6)(*[u.data_ptr() for u in ups])
            hip.check(lib.catre_loss_bwd_sums(*head, p(x["is_sym"]), p(best), p(counts), p(up), parr, terms, 6, ctypes.byref(c),
                                              p(dpose), p(dscale), B, M, S1, st), "catre_loss_bwd_sums")
        else:
            hip.check(lib.catre_loss_bwd(*head, p(x["is_sym"]), p(best), p(counts), p(up), ctypes.byref(c), p(dpose), p(dscale),
                                         B, M, S1, st), "catre_loss_bwd")
        torch.cuda.synchronize()
        out.update({f"{tag}_losses": bits(losses), f"{tag}_best": best.cpu().numpy(), f"{tag}_counts": counts.cpu().numpy(),
                    f"{tag}_dpose": bits(dpose), f"{tag}_dscale": bits(dscale)})
        if sums:
            out["sums_prefix"] = bits(prefix)
    return out


def compare(got, want):
    bad = [k for k in want if not np.array_equal(np.asarray(got[k]), np.asarray(want[k]))]
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write")
    ap.add_argument("--check")
    a = ap.parse_args()
    got = run_old_entry_points()
    if a.write:
        np.savez_compressed(a.write, **got)
        print("wrote", a.write, {k: v.shape for k, v in got.items()})
    if a.check:
        want = dict(np.load(a.check))
        bad = compare(got, want)
        print("bit-identical:" if not bad else "DIFFERENT:", sorted(want) if not bad else bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
