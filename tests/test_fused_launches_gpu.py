"""The launch trace of one FusedStepper iteration (capture=False): every call into the library with every argument, every event
record and every stream wait, in issue order, against tests/golden/fused_launch_traces.json.  The golden was recorded by this
file's own recorder (`python tests/test_fused_launches_gpu.py`, which rewrites it) on the commit BEFORE FusedStepper took its
scheduling decisions from `launch_plan`: a change of homan_amd/fused.py that keeps the launches keeps this test green, and
the file is not regenerated for such a change.  GPU box."""
import contextlib
import copy
import ctypes
import hashlib
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import util  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(util.GOLDEN_DIR, "fused_launch_traces.json")


def _prototypes():
    """entry point -> [(parameter name, 'stream' | 'ptr' | 'float' | 'int')], read off include/homan_amd.h"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "homan_amd.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(hm_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        params = [] if m.group(2).strip() == "void" else m.group(2).split(",")
        out[m.group(1)] = [(re.search(r"(\w+)\s*$", p).group(1),
                            "stream" if "hipStream_t" in p else "ptr" if "*" in p else
                            "float" if re.search(r"\b(float|double)\b", p) else "int") for p in params]
    return out


class _Proxy:
    """passes every call on to the loaded library and writes it down first"""

    def __init__(self, real, events):
        self._real, self._events = real, events

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self._events.append(("call", name, args))
            return fn(*args)
        return call


@contextlib.contextmanager
def _recording(events):
    """`homan_amd.lib.lib()` returns the proxy, Event.record / Stream.wait_event / Stream.wait_stream write themselves down;
    everything is put back on the way out"""
    from homan_amd import lib as hlib
    real_lib, proxy = hlib.lib, _Proxy(hlib.lib(), events)
    E, S = torch.cuda.Event, torch.cuda.Stream
    real = (E.record, S.wait_event, S.wait_stream)
    inside = []          # (torch's wait_stream is an event record + wait of its own: not ours)

    def record(self, stream=None):
        if not inside:
            events.append(("record", stream if stream is not None else torch.cuda.current_stream(), self))
        return real[0](self) if stream is None else real[0](self, stream)

    def wait_event(self, event):
        if not inside:
            events.append(("wait", self, event))
        return real[1](self, event)

    def wait_stream(self, stream):
        if not inside:
            events.append(("wait_stream", self, stream))
        inside.append(1)
        try:
            return real[2](self, stream)
        finally:
            inside.pop()
    hlib.lib = lambda: proxy
    E.record, S.wait_event, S.wait_stream = record, wait_event, wait_stream
    try:
        yield
    finally:
        hlib.lib = real_lib
        E.record, S.wait_event, S.wait_stream = real


def _device_tensors(root):
    """[(path, tensor)] of the device tensors reachable from the stepper (its model, contexts, optimiser), gradients included,
    walked in ONE order: attributes and keys sorted by name, sequences by index"""
    out, seen = [], set()

    def walk(obj, path, depth):
        if isinstance(obj, torch.Tensor):
            if obj.is_cuda and obj.numel() and obj.is_contiguous():
                out.append((path, obj))
            if obj.grad is not None:
                walk(obj.grad, path + ".grad", depth)
            return
        if id(obj) in seen or depth > 10:
            return
        seen.add(id(obj))
        if isinstance(obj, dict):
            items = sorted((str(k), v) for k, v in obj.items())
        elif isinstance(obj, (list, tuple)):
            items = [(str(i), v) for i, v in enumerate(obj)]
        elif hasattr(obj, "__dict__") and type(obj).__module__.split(".")[0] == "homan_amd":
            items = sorted(vars(obj).items())
        else:
            return
        for k, v in items:
            walk(v, path + "." + k, depth + 1)
    walk(root, "st", 0)
    return out


def _format(st, main, events):
    """-> (readable sequence, full text): one line per call / record / wait"""
    from homan_amd import lib as hlib
    protos, tensors = _prototypes(), _device_tensors(st)
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), path) for path, t in tensors]
    streams = {main.cuda_stream: "main", st.side.cuda_stream: "side", st.aux.cuda_stream: "aux"}
    assert len(streams) == 3
    names = {id(v): k for k, v in vars(st).items() if isinstance(v, torch.cuda.Event)}

    def stream(s):
        handle = s.cuda_stream if isinstance(s, torch.cuda.Stream) else (s or 0)
        assert handle in streams, "a stream that is none of the stepper's"
        return streams[handle]

    def pointer(a):
        a = a.value if isinstance(a, ctypes.c_void_p) else a
        if not a:
            return "NULL"
        best = None
        for lo, hi, path in spans:                # the buffer that starts closest below the address; the first in walk order
            if lo <= a < hi and (best is None or a - lo < best[0]):
                best = (a - lo, path)
        assert best is not None, "a device pointer that belongs to no tensor reachable from the stepper"
        return "%s+%d" % (best[1], best[0])

    def value(a, kind):
        if isinstance(a, ctypes.Array):           # host arrays, element by element
            if issubclass(a._type_, ctypes.Structure):
                kinds = {ctypes.c_void_p: "ptr", ctypes.c_float: "float"}
                return "[" + ",".join("{" + ",".join("%s=%s" % (f, value(getattr(r, f), kinds.get(ct, "int")))
                                                     for f, ct in hlib.SilRender._fields_) + "}" for r in a) + "]"
            return "[" + ",".join(value(x, "float" if a._type_ is ctypes.c_float else "ptr") for x in a) + "]"
        if kind == "ptr":
            return pointer(a)
        return float(a).hex() if kind == "float" else "%d" % a

    short, full = [], []
    for ev in events:
        if ev[0] == "call":
            _, name, args = ev
            params = protos[name]
            assert len(params) == len(args), name
            on = [stream(a) for (_, kind), a in zip(params, args) if kind == "stream"]
            head = "%s %s" % (on[0] if on else "-", name)
            short.append(head)
            full.append(head + "".join(" %s=%s" % (n, value(a, kind)) for (n, kind), a in zip(params, args) if kind != "stream"))
        else:
            what, s, other = ev
            assert what == "wait_stream" or id(other) in names, "an event that is none of the stepper's"
            line = "%s %s %s" % (stream(s), what, stream(other) if what == "wait_stream" else names[id(other)])
            short.append(line)
            full.append(line)
    return short, "\n".join(full) + "\n"


# ---------------------------------------------------------------- the configurations: the smallest that still take each branch
def _synth_models(mano, seeds=(0,), size=64, obj="cube", hands=("right",), **kw):
    from homan_amd import synth
    from homan_amd.jointopt import build_model
    sil_fn, hand_fn = synth.hip_clip_fns(mano)
    models = []
    for seed in seeds:
        clip = synth.make_clip(seed=seed, frames=2, rend_size=size, image_size=size, obj=obj, silhouette_fn=sil_fn,
                               hand_verts_fn=hand_fn, hands=hands)
        models.append(build_model(copy.deepcopy(clip["person_parameters"]), copy.deepcopy(clip["object_parameters"]),
                                  objvertices=clip["objvertices"], objfaces=clip["objfaces"], camintr=clip["camintr"],
                                  image_size=size, mano_model=mano, rend_size=size, sync_metrics=False,
                                  **dict(dict(optimize_mano=True), **kw)))
    return models if len(models) > 1 else models[0]


def _golden_model(mano, name):
    from homan_amd import HOMan
    _, inputs, camintr, weights, meta = util.load_golden(name)
    return HOMan(mano_model=mano, rend_size=meta["image_size"], sync_metrics=False, **util.model_kwargs(inputs, camintr, meta)), weights


def _configs():
    """name -> (mano -> (model or list of models, loss weights, FusedStepper keywords))"""
    from homan_amd import synth
    S1, S2, C1 = dict(synth.STEP1_LOSS_WEIGHTS), dict(synth.STEP2_LOSS_WEIGHTS), dict(synth.CFG1_LOSS_WEIGHTS)
    S1D = dict(S1, lw_depth=2.0)
    bottle = lambda seg, rings: synth.bottle_mesh(segments=seg, rings=rings)
    golden = lambda name: (lambda mano: _golden_model(mano, name) + ({},))
    return {
        "cfg1": lambda mano: (_synth_models(mano), C1, {}),
        "step1": lambda mano: (_synth_models(mano), S1, {}),
        "step2": lambda mano: (_synth_models(mano), S2, {}),
        "step1_depth_s64": lambda mano: (_synth_models(mano, ordinal_depth=True), S1D, {}),            # Sd % 64 == 0: flags
        "step1_depth_s32": lambda mano: (_synth_models(mano, size=32, ordinal_depth=True), S1D, {}),   # no flags
        "step1_2clips": lambda mano: (_synth_models(mano, (0, 1)), S1, {}),
        "step2_2clips": lambda mano: (_synth_models(mano, (0, 1)), S2, {}),
        "step2_2clips_shared_scale": lambda mano: (_synth_models(mano, (0, 1), optimize_object_scale=True), S2,
                                                   dict(shared_scale=True)),
        "step1_depth_2clips": lambda mano: (_synth_models(mano, (0, 1), ordinal_depth=True), S1D, {}),
        "step2_free_scale": golden("ref_step2_scale_bottle_b5_s64"),
        "inter_min": golden("ref_step2_intermin_cube_b4_s64"),
        "optimize_mano_off": golden("ref_rigid_cube_b5_s32"),
        "left_hand": golden("ref_step1_lefthand_cube_b4_s64"),
        "two_hands_step2": golden("ref_step2_twohands_cube_b4_s64"),
        "two_hands_depth": lambda mano: (_synth_models(mano, hands=("right", "left"), ordinal_depth=True),
                                         dict(S2, lw_depth=2.0), {}),
        "step1_vo4502": lambda mano: (_synth_models(mano, obj=bottle(90, 50)), S1, {}),
        "step1_vo25002": lambda mano: (_synth_models(mano, obj=bottle(200, 125)), S1, {}),
    }


CONFIGS = ["cfg1", "step1", "step2", "step1_depth_s64", "step1_depth_s32", "step1_2clips", "step2_2clips",
           "step2_2clips_shared_scale", "step1_depth_2clips", "step2_free_scale", "inter_min", "optimize_mano_off", "left_hand",
           "two_hands_step2", "two_hands_depth", "step1_vo4502", "step1_vo25002"]


def _trace(name, mano):
    from homan_amd.jointopt import FusedStepper
    model, weights, kw = _configs()[name](mano)
    events = []
    with _recording(events):
        st = FusedStepper(model, weights, 1e-2, 4, capture=False, **kw)
        torch.cuda.synchronize()
        del events[:]                     # (construction and its warm-up are not the iteration)
        main = torch.cuda.current_stream()
        st._iteration()
        torch.cuda.synchronize()
    return _format(st, main, events)


@pytest.mark.parametrize("name", CONFIGS)
def test_one_iteration_issues_the_recorded_launches(name, mano_model, tmp_path):
    assert sorted(CONFIGS) == sorted(_configs())
    with open(GOLDEN) as fh:
        want = json.load(fh)[name]
    short, full = _trace(name, mano_model)
    if short != want["sequence"] or hashlib.sha256(full.encode()).hexdigest() != want["sha256"]:
        path = tmp_path / (name + ".trace.txt")
        path.write_text(full)
        first = next((i for i, (a, b) in enumerate(zip(short, want["sequence"])) if a != b), min(len(short), len(want["sequence"])))
        where = ("line %d: issued `%s`, recorded `%s`" % (first + 1, (short + ["(end)"])[first], (want["sequence"] + ["(end)"])[first])
                 if short != want["sequence"] else "same sequence, an argument differs")
        pytest.fail("%s: launch trace differs from tests/golden/fused_launch_traces.json - %s; the full trace of this run: %s"
                    % (name, where, path))


if __name__ == "__main__":
    # the recorder: rewrites the golden from the checkout this file lies in (with --full DIR: the full texts too, for reading)
    from homan_amd.mano_assets import synthetic_mano
    mano, out = synthetic_mano(0), {}
    full_dir = sys.argv[sys.argv.index("--full") + 1] if "--full" in sys.argv else None
    for cfg in CONFIGS:
        seq, text = _trace(cfg, mano)
        out[cfg] = dict(sequence=seq, sha256=hashlib.sha256(text.encode()).hexdigest())
        if full_dir:
            os.makedirs(full_dir, exist_ok=True)
            with open(os.path.join(full_dir, cfg + ".trace.txt"), "w") as fh:
                fh.write(text)
        print(cfg, len(seq), "lines", out[cfg]["sha256"][:12], flush=True)
    with open(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")
