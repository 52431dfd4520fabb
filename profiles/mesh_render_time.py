"""Time of the mesh rasteriser (``render.render_mesh``, ``csrc/catre_mesh.h``) on the GPU:

    python profiles/mesh_render_time.py --out profiles     # profiles/mesh_render_time.json

``catre_mesh_render`` through the C ABI on preallocated buffers - all outputs, ``coord`` included, so a call is the table copy
and four launches (clear, project, raster, resolve) - with the protocol of ``profiles/splat_time.py`` and its scene: I = 256
objects spread over F = 16 frames of 480x640 (16 per frame, 0.5 - 1.2 m), with an observed depth, and I = 1, F = 1; the mesh
is an ``icosphere`` of 1 280 and of 20 480 faces (radius 0.5, scaled like the splat's boxes), shared by all instances.  HIP
events around ``--reps`` back-to-back calls after a warm-up, five windows, the median window and the spread between the windows
are quoted.  Next to it, in the same process, ``catre_splat_render`` at M = 1024 points on the same poses
(``splat_time.splat_time``).

``per_launch_us`` splits a call into its kernels with the device-side durations ``torch.profiler`` records over 20 calls
(it traces, so these calls are not the timed ones); null with the reason if the profiler is not available."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import splat_time as ST  # noqa: E402

H, W, DELTA = ST.H, ST.W, ST.DELTA


def per_launch(call, n=20):
    import torch

    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(n):
                call()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None)
            if t is None:
                t = getattr(e, "cuda_time_total", 0.0)
            if e.key.startswith(("k_mesh_", "k_splat", "k_zbuf_")) and t > 0:
                out[e.key.split("(")[0]] = round(t / n, 3)
        return out or dict(error="the profiler recorded no kernel of the call")
    except Exception as err:  # the split is an extra: the timing above it stands without it
        return dict(error=f"{type(err).__name__}: {err}")


def mesh_time(subdiv, I, F, reps):
    import torch

    from catre_amd import hip, meshes as MS

    lib = hip.load()
    _, pose, scale, K, frame_of, depth = ST.scene(I, F, seed=I)
    pose, scale, depth = (torch.as_tensor(a).cuda() for a in (pose, scale, depth))
    ms = MS.MeshSet.from_list([MS.icosphere(subdiv, 0.5)], "cuda", mesh_of=[0] * I)
    ivo, ifo = ms.instance_offsets()
    NV, NF = int(ivo[-1]), int(ifo[-1])
    off = torch.from_numpy(np.stack([ivo, ifo]).astype(np.int32)).cuda()
    nbytes = lib.catre_mesh_workspace_bytes(F, H, W, NV)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")
    labels, face, fit, counts, culled = i32(F, H, W), i32(F, H, W), i32(F, H, W), i32(I, 5), i32(I)
    zbuf = torch.empty(F, H, W, device="cuda")
    cls = torch.empty(F, H, W, dtype=torch.uint8, device="cuda")
    coord = torch.empty(F, H, W, 3, device="cuda")
    k9 = (ctypes.c_float * (9 * F))(*[float(v) for v in np.tile(K.reshape(-1), F)])
    fo = (ctypes.c_int32 * I)(*frame_of)
    st = hip.stream_ptr(pose.device)

    def call():
        hip.check(lib.catre_mesh_render(hip.ptr(ms.verts), hip.ptr(ms.faces), hip.ptr(ms.vert_off), hip.ptr(ms.face_off),
                                        hip.ptr(ms.mesh_of), hip.ptr(off[0]), hip.ptr(off[1]), hip.ptr(pose), hip.ptr(scale),
                                        hip.ptr(depth), k9, fo, DELTA, 0, 1, ms.v_tot, ms.t_tot, F, I, NV, NF, H, W, hip.ptr(ws), nbytes,
                                        hip.ptr(labels), hip.ptr(zbuf), hip.ptr(face), hip.ptr(cls), hip.ptr(fit), hip.ptr(counts),
                                        hip.ptr(culled), hip.ptr(coord), ctypes.c_void_p(0), st), "catre_mesh_render")

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    w = ST.windows(call, reps)
    ms_call = float(np.median(w))
    rendered = int((labels > 0).sum().item())
    cnt = counts.sum(0).tolist()
    assert cnt[0] == rendered == sum(cnt[1:])
    return dict(instances=I, faces_per_mesh=ms.t_tot, posed_faces=NF, posed_vertices=NV, frames=F, frame=f"{H}x{W}",
                ms_per_call=round(ms_call, 5), ms_windows=[round(x, 5) for x in w],
                window_spread=round((max(w) - min(w)) / ms_call, 4), calls_per_window=reps, rendered_pixels_per_call=rendered,
                culled_faces=int(culled.sum().item()), pixels_per_face=round(rendered / NF, 3),
                m_posed_faces_per_s=round(NF / ms_call / 1e3, 2), per_launch_us=per_launch(call))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small-reps", type=int, default=300)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    import torch

    assert torch.cuda.is_available(), "mesh_render_time.py measures on a HIP device"
    res = dict(what="catre_mesh_render", device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
               delta=DELTA,
               mesh=[mesh_time(3, 256, 16, a.reps), mesh_time(5, 256, 16, a.reps), mesh_time(3, 1, 1, a.small_reps),
                     mesh_time(5, 1, 1, a.small_reps)],
               splat=[ST.splat_time(256, 16, True, a.reps), ST.splat_time(1, 1, True, a.small_reps)],
               note="HIP events around back-to-back C-ABI calls on preallocated buffers after 10 warm-up calls, all outputs written "
                    "(coord included): one table copy and four launches per call; the median of five windows, window_spread = "
                    "(max - min) / median.  rendered_pixels counts the pixels that end up covered, a lower bound of the 64-bit "
                    "atomicMin count (a visible pixel is covered by one front face and usually one back face: there is no "
                    "back-face culling).  per_launch_us: device-side kernel durations from a traced run of 20 calls.  splat: "
                    "catre_splat_render at 1024 points per instance on the same poses, same process")
    json.dump(res, open(os.path.join(a.out, "mesh_render_time.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
