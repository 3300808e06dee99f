"""Phases of the critical workgroup of the iteration's two tail kernels - k_rigid_bwd_x (csrc/geometry.hip) and k_mano_bwd
(csrc/mano.hip) - INSIDE the replayed graph, at cfg2 (30 frames) and at ONE frame of the same clip (tools/ledger.sh shapes).
Debug build: tools/ab_build.sh tail -DHM_CHAIN_STAMPS -DMANO_PHASES; HOMAN_AMD_LIB=variants/lib_tail.so python tools/tail_phases.py
[--out FILE.json].  Every mark is the LATEST arrival of any workgroup of the launch at that point (hm_common.h HM_PH: taken once
what was requested before it has landed, which serialises a little: the sum of the phases is longer than the release kernel), in
microseconds from the launch's first workgroup start; medians over single replays.  GPU box."""
import argparse, copy, ctypes, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap = argparse.ArgumentParser(); ap.add_argument("--out", default=None); ap.add_argument("--warm", type=int, default=300)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
import numpy as np, torch
from homan_amd import lib as hlib, synth
from homan_amd.jointopt import FusedStepper, build_model
from homan_amd.mano_assets import synthetic_mano

RIGID = ["start", "vertex loads (offsets)", "corner items", "corner sums", "block sum", "record stored", "ticket", "records reloaded",
         "finish"]
MANO = ["start", "state + vertex loads", "chunk sums + skinning", "dA + rows + records", "ticket", "partials + tables reloaded",
        "level loop", "Rodrigues, betas, rot6d", "PCA"]
mano = synthetic_mano(0)
sil_fn, hand_fn = synth.hip_clip_fns(mano)
L = hlib.lib()
for f in ("hm_debug_tail_geometry", "hm_debug_tail_mano"):
    getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_int]
result = {}
for name, frames, lw in (("cfg2", 30, synth.STEP1_LOSS_WEIGHTS), ("one_frame", 1, synth.CFG1_LOSS_WEIGHTS)):
    c = synth.make_clip(seed=0, frames=frames, rend_size=256, image_size=256, obj="bottle", silhouette_fn=sil_fn, hand_verts_fn=hand_fn)
    m = build_model(copy.deepcopy(c["person_parameters"]), copy.deepcopy(c["object_parameters"]), objvertices=c["objvertices"],
                    objfaces=c["objfaces"], camintr=c["camintr"], optimize_mano=True, image_size=256, mano_model=mano, rend_size=256,
                    sync_metrics=False)
    st = FusedStepper(m, dict(lw), 1e-2, args.warm + 100)
    st.run(args.warm)
    rows = {"k_rigid_bwd_x": [], "k_mano_bwd": []}
    for rep in range(args.reps):
        L.hm_debug_tail_geometry(None, 1); L.hm_debug_tail_mano(None, 1)
        st.run(1)
        torch.cuda.synchronize()
        for key, fn in (("k_rigid_bwd_x", L.hm_debug_tail_geometry), ("k_mano_bwd", L.hm_debug_tail_mano)):
            o = (ctypes.c_ulonglong * 16)()
            fn(o, 0)
            rows[key].append([(int(o[k]) - int(o[15])) / 100.0 if o[k] else float("nan") for k in range(9)])
    result[name] = {}
    for key, names in (("k_rigid_bwd_x", RIGID), ("k_mano_bwd", MANO)):
        med = np.nanmedian(np.asarray(rows[key]), axis=0)
        result[name][key] = {n: (None if np.isnan(v) else round(float(v), 2)) for n, v in zip(names, med)}
        print(name, key, "  ".join(f"{n}={v:.2f}" for n, v in zip(names, med)))
    del st, m
if args.out:
    json.dump(result, open(args.out, "w"), indent=1)
