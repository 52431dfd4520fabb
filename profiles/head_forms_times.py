"""Times of the generic norm + activation ops (csrc/catre_heads.h) at B = 256 objects, P = 2048 points, C in {128, 256, 512}
(GroupNorm with 32 groups, every activation), next to the ops specialised for (256 channels, 32 groups, GELU) at C = 256 in
the same process:

    python profiles/head_forms_times.py [profiles/head_forms_kernel_times.json]      # on the GPU

Per op: device events around ITERS back-to-back calls after WARM warm-up calls, the median of REPS such windows; one call is
the op's whole launch chain (statistics + merge + apply for the forward).  GB/s is against the bytes the op MUST move,
computed from the shape: forward reads Y and writes A once each (2 x rows x C x 4 bytes; its statistics pass reads Y a second
time - that is not in the figure, which is why a forward cannot reach the copy rate); backward reads dA and Y and writes dY
(3 x); the fused tail reads Y once.  A record, not a bar.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, P, G = 256, 2048, 32
WIDTHS = (128, 256, 512)
WARM, ITERS, REPS = 3, 10, 5


def _time(fn):
    import torch

    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / ITERS)
    return statistics.median(ms) * 1e3   # us


def run(out):
    import torch

    from catre_amd import hip
    from catre_amd import train_ops as T

    dev = "cuda:0"
    acts = dict(relu=hip.ACT_RELU, lrelu=hip.ACT_LRELU, silu=hip.ACT_SILU, gelu=hip.ACT_GELU, mish=hip.ACT_MISH,
                none=hip.ACT_NONE)
    res = {"shape": {"B": B, "P": P, "groups": G}, "unit": "us per call (median of %d windows of %d calls)" % (REPS, ITERS),
           "device": torch.cuda.get_device_name(0), "ops": []}

    def rec(op, C, act, norm, us, passes):
        nbytes = passes * B * P * C * 4
        res["ops"].append(dict(op=op, C=C, act=act, norm=int(norm), us=round(us, 1), bytes=nbytes,
                               GBps=round(nbytes / us / 1e3, 1)))
        print(res["ops"][-1])

    g = torch.Generator().manual_seed(0)
    for C in WIDTHS:
        y = torch.randn(B * P, C, generator=g).to(dev)
        da = torch.randn(B * P, C, generator=g).to(dev)
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        wn, bn = torch.randn(3, C, 1, device=dev) * 0.01, torch.zeros(3, device=dev)
        wp, bp = torch.full((1, P, 1), 1.0 / P, device=dev), torch.zeros(1, device=dev)
        for act, aid in acts.items():
            for norm in ((True, False) if act in ("gelu", "relu") else (True,)):
                ga, be = (gamma, beta) if norm else (None, None)
                with torch.no_grad():
                    rec("gnp_act_fwd", C, act, norm, _time(lambda: T.gn_points_act(y, ga, be, B, P, G, aid, norm)), 2)
                    rec("gnp_act_neck_wsum", C, act, norm,
                        _time(lambda: T.gn_points_act_neck_wsum(y, ga, be, wn, bn, wp, bp, B, P, G, aid, norm)), 1)
                yl = y.clone().requires_grad_(True)
                a = T.gn_points_act(yl, ga, be, B, P, G, aid, norm)
                rec("gnp_act_bwd", C, act, norm, _time(lambda: torch.autograd.grad(a, yl, da, retain_graph=True)), 3)
                del a, yl
        if C == 256:   # the ops written for this one shape, same process, same buffers
            with torch.no_grad():
                rec("gnp_gelu_fwd (specialised)", C, "gelu", True, _time(lambda: T.gn_points_gelu(y, gamma, beta, B, P)), 2)
            yl = y.clone().requires_grad_(True)
            a = T.gn_points_gelu(yl, gamma, beta, B, P)
            rec("gnp_gelu_bwd (specialised)", C, "gelu", True, _time(lambda: torch.autograd.grad(a, yl, da, retain_graph=True)), 3)
            del a, yl
        # the row form at the ts head's size: B rows
        yr = y[:B].contiguous()
        with torch.no_grad():
            us = _time(lambda: T.gn_rows_act(yr, gamma, beta, G, hip.ACT_GELU, True))
        res["ops"].append(dict(op="gnr_act_fwd", C=C, act="gelu", norm=1, rows=B, us=round(us, 1)))
        print(res["ops"][-1])
        del y, da
    gen = [o for o in res["ops"] if o["op"] == "gnp_act_fwd" and o["C"] == 256 and o["act"] == "gelu" and o["norm"] == 1][0]
    spec = [o for o in res["ops"] if o["op"].startswith("gnp_gelu_fwd")][0]
    res["generic_over_specialised_fwd_c256_gelu"] = round(gen["us"] / spec["us"], 3)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("generic / specialised forward at C=256:", res["generic_over_specialised_fwd_c256_gelu"])


if __name__ == "__main__":
    run(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "head_forms_kernel_times.json"))
