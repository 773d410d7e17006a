"""Captured train steps: the device part of a step (trainer.TrainStep._device_step) recorded once per configuration into a
hipGraph and replayed -- as the graph, or as a launch plan of the library (csrc/svs_plan.hip) -- with the inputs of every step
uploaded into the capture's static tensors."""
import ctypes
import gc
import os
import sys
import warnings

import torch

from . import lib as _lib
from . import ops


class _LaunchPlan:
    """The launch sequence of a captured step as a plan of the library (csrc/svs_plan.hip): the capture's nodes and edges
    read once, then enqueued per step by one call -- plain launches on the step's stream topology, no hipGraphLaunch, no
    interpreter between the launches (the call releases the GIL)."""

    def __init__(self, graph, side_streams=()):
        self._lib, self._check = _lib.load(), _lib.check
        self.graph = graph                               # the kernel arguments live in the graph's nodes
        self.side_streams = list(side_streams)           # torch streams the side chains run on (kept alive here)
        arr = (ctypes.c_void_p * max(1, len(self.side_streams)))(*[s.cuda_stream for s in self.side_streams])
        handle = ctypes.c_void_p()
        self._check(self._lib.svs_plan_build(ctypes.c_void_p(int(graph.raw_cuda_graph())), arr, len(self.side_streams),
                                       ctypes.byref(handle)), "svs_plan_build")
        self.handle = handle
        counts = (ctypes.c_int * 8)()
        self._check(self._lib.svs_plan_info(handle, counts), "svs_plan_info")
        self.info = dict(zip(("nodes", "kernels", "copies", "memsets", "empty", "streams", "events", "entry_streams"),
                             list(counts)))

    def describe(self):
        """one line per node, in issue order (stream, kernel name and launch shape, events waited for / recorded)"""
        buf = ctypes.create_string_buffer(1 << 18)
        self._check(self._lib.svs_plan_describe(self.handle, buf, len(buf)), "svs_plan_describe")
        return buf.value.decode()

    def run(self):
        self._check(self._lib.svs_plan_run(self.handle, torch.cuda.current_stream().cuda_stream), "svs_plan_run")

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                self._lib.svs_plan_destroy(h)
            except Exception:
                pass



class _CapturedStep:
    """One captured launch sequence (hipGraph) of the device part of a step, with the static tensors it reads."""

    def __init__(self):
        self.graph = None
        self.plan = None            # graph == "plan": the capture replayed as eager launches by the library
        self.static = {}            # name -> persistent device tensor (inputs, random draws, step-varying scalars)
        self.scratch = None
        self.result = None          # what the eager step would have returned: tensors inside the graph's pool
        self.hold = None
        self.calls = 0

    def upload(self, ts, model_input, ground_truth, mvs, n_valid):
        """Host -> static tensors of a captured step, on the current stream (ordered before the replay).  Everything
        except the random draws -- pixels, camera, target colours, the two annealing scalars, the rendered-view index --
        has a fixed place in ONE static device buffer and travels in one transfer from a 4-deep ring of pinned staging
        buffers (the host waits for the transfer made FOUR steps ago, i.e. never in practice: with one staging buffer it
        waited for the previous step's, which sits behind that step's kernels -- host and GPU took turns).  An input that
        already lives on the device is copied into its place by a device copy behind the transfer."""
        st = self.static
        dev = ts.fp.flat.device
        annealed, anneal_sparse = ts.loss.anneal_state()
        target = ground_truth["rgb_smooth"] if annealed else ground_truth["rgb"]
        origin = {k: model_input[k] for k in ("uv", "intrinsics", "pose")}
        origin["target"] = target
        pieces = [(k, model_input[k]) for k in ("uv", "intrinsics", "pose")] + [("target", target.reshape(-1, 3))]
        if "_all" not in st:
            off = 4                                          # words 0..1: annealing state, word 2: rendered-view index (int32)
            st["_layout"] = {}
            for k, src in pieces:
                st["_layout"][k] = (off, tuple(src.shape))
                off += (src.numel() + 3) // 4 * 4            # 16-byte aligned pieces
            st["_all"] = torch.zeros(off, dtype=torch.float32, device=dev)
            st["_ring"] = [dict(pin=torch.zeros(off, dtype=torch.float32).pin_memory(), ev=None) for _ in range(4)]
            st["_i"] = 0
            for k, (o, shape) in st["_layout"].items():
                n = 1
                for d in shape:
                    n *= d
                st[k] = st["_all"][o:o + n].view(shape)
            st["anneal"] = st["_all"][0:2]
            st["same_view"] = st["_all"][2:3].view(torch.int32)
            st["rng"] = {}
        slot = st["_ring"][st["_i"] % 4]
        st["_i"] += 1
        if slot["ev"] is not None:
            slot["ev"].synchronize()
        pin = slot["pin"]
        pin[0] = 1.0 if annealed else 0.0
        pin[1] = float(anneal_sparse)
        pin[2:3].view(torch.int32)[0] = int(mvs["same_view"]) if mvs is not None else -1
        on_device, host = [], False
        seen = st.setdefault("_seen", {})
        for k, src in pieces:
            o, shape = st["_layout"][k]
            if tuple(src.shape) != shape:
                raise ValueError(f"captured step: input {k} changed shape {shape} -> {tuple(src.shape)}")
            if src.is_cuda:
                # a device tensor the caller hands over unchanged step after step is in place: the SAME tensor object (kept
                # referenced here, so its storage cannot have been handed to another tensor) at the same version
                tag = (origin[k], origin[k]._version)
                old = seen.get(k)
                if old is None or old[0] is not tag[0] or old[1] != tag[1]:
                    on_device.append((k, src, tag))
            else:
                pin[o:o + src.numel()].copy_(src.reshape(-1))
                host = True
                seen.pop(k, None)
        head = (float(pin[0]), float(pin[1]), int(pin[2:3].view(torch.int32)[0]))
        if host:
            # (pieces that live on the device keep their place in the static buffer: the transfer writes their region of the
            # staging buffer -- stale -- over them, so they are copied again behind it)
            if any(src.is_cuda for _, src in pieces):
                on_device = [(k, src, (origin[k], origin[k]._version)) for k, src in pieces if src.is_cuda]
            ops.stage_in(st["_all"], pin)
        elif st.get("_head") != head:
            ops.stage_in(st["_all"][:4], pin[:4])                  # the three scalars only
        if host or st.get("_head") != head:
            slot["ev"] = torch.cuda.Event()
            slot["ev"].record()
            st["_head"] = head
        for k, src, tag in on_device:
            st[k].copy_(src, non_blocking=True)
            seen[k] = tag
        # (as the eager step: a data-parallel rank draws for the whole batch and keeps its rays' rows; a padded batch
        # consumes the random stream of the caller's rays)
        ts.model.draw_rays(n_valid, model_input["uv"].shape[1], dev, *ts._draw_shard(), out=st["rng"])



class CapturedSteps(dict):
    """capture key -> _CapturedStep of one TrainStep `ts` (its `_captured`): at most four configurations, captured into one graph
    memory pool on one capture stream."""

    def __init__(self):
        super().__init__()
        self._graph_pool = None
        self._capture_stream = None
        self._evicted = None

    def key(self, ts, model_input, mvs, fast, n_valid):
        R = model_input["uv"].shape[1]
        mk = None
        if mvs is not None:
            # everything ops.cost_lookup hands to the kernel BY VALUE is baked into the capture: the cost / z range
            # addresses and shapes, and the camera parameters of every view (an MVS re-run can return a re-used address
            # with different cameras)
            def view_key(v):
                ptrs = tuple((int(v[k].data_ptr()), tuple(v[k].shape)) for k in ("cost", "z_mvs") if torch.is_tensor(v.get(k)))
                cams = []
                for k in sorted(v):
                    if k in ("cost", "z_mvs"):
                        continue
                    x = v[k]
                    if torch.is_tensor(x):
                        cams.append((k, int(x.data_ptr()), x._version, tuple(x.shape)))
                    else:
                        cams.append((k, repr(x)))
                return ptrs, tuple(cams)
            mk = (len(mvs["views"]), tuple(mvs["img_res"]), bool(mvs.get("inverse_depth", False)),
                  tuple(view_key(v) for v in mvs["views"]))
        return (R, n_valid, tuple(ts._groups_for(R, n_valid)), fast, mk, str(ts.fp.flat.device), ts.graph)

    def step(self, ts, model_input, ground_truth, mvs, fast, n_valid):
        """-> results of the step (replayed from its graph), or None when this call has to run eagerly: the first step of
        a configuration runs eagerly (it also performs the one-time kernel attribute set-up), the second is captured."""
        key = self.key(ts, model_input, mvs, fast, n_valid)
        cs = self.get(key)
        if cs is None:
            if len(self) >= 4:                 # a few configurations at most (stages, render previews)
                # the evicted graph's result tensors may still be the caller's: it is destroyed one step later
                self._evicted = self.pop(next(iter(self)))
            cs = self[key] = _CapturedStep()
        cs.calls += 1
        if cs.calls == 1:
            return None
        m = ts.model
        cs.upload(ts, model_input, ground_truth, mvs, n_valid)
        ts._draws_done()
        if cs.graph is None:
            st = cs.static
            cs.scratch = ts._new_scratch()
            inp = dict(model_input)
            inp.update(uv=st["uv"], intrinsics=st["intrinsics"], pose=st["pose"])
            gt = {"rgb": st["target"], "rgb_smooth": st["target"]}
            dyn = dict(same_view=st["same_view"], anneal=st["anneal"])
            # one eager pass over the capture's own scratch first: what a step allocates once and keeps (the backward's blocks,
            # zero-initialised: ~1 GB per 256 rays) must exist BEFORE the recording -- allocated inside it, the zero fills would
            # be recorded as launches and repeated by every replay (that, not the replay mechanism, was what made the captured
            # step of round 3 slower than the eager one)
            # -- on the stream the recording will run on: the model keeps per-stream workspaces (the sampler's, the side
            # streams of the background networks), which would otherwise be created, and zero-filled, inside the recording
            if self._capture_stream is None:
                self._capture_stream = torch.cuda.Stream(device=ts.fp.flat.device)
            cap = self._capture_stream
            cap.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(cap):
                ts._device_step(cs.scratch, inp, gt, mvs, fast, st["rng"], dyn, serial=ts.graph == "linear", n_valid=n_valid)
            torch.cuda.current_stream().wait_stream(cap)
            m.invalidate_packed()                        # the capture must contain the weight packing
            plan_mode = ts.graph in ("plan", "auto")
            # (keep_graph: the capture stays a hipGraph_t that svs_plan_build can read; it is never instantiated)
            graph = torch.cuda.CUDAGraph(keep_graph=True) if plan_mode else torch.cuda.CUDAGraph()
            if self._graph_pool is None:
                self._graph_pool = torch.cuda.graph_pool_handle()
            # (thread_local: a helper thread that prepares the next batch meanwhile -- VolOpt.run -- does not disturb the capture)
            # No cyclic garbage collection while the recording runs: a collection that finds an earlier TrainStep's
            # capture (a graph + its memory pool) would free device memory in the middle of this one, which the runtime
            # refuses -- from a destructor, i.e. the process aborts.  (torch.cuda.graph collects once on entry.)
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(graph, pool=self._graph_pool, stream=cap, capture_error_mode="thread_local"):
                    cs.result, cs.hold = ts._device_step(cs.scratch, inp, gt, mvs, fast, st["rng"], dyn,
                                                         serial=ts.graph == "linear", n_valid=n_valid)
            finally:
                if gc_was_on:
                    gc.enable()
            cs.graph = graph
            if plan_mode:
                # the side chains run on streams of the capture's own scratch (torch pool streams, as in the eager schedule)
                sc = cs.scratch
                side = ([sc.prep] + list(sc.sides) + [b._side for b in sc.bwd] + list(getattr(m, "_bg_streams", {}).values())
                        + list(sc._bg_streams.values()))
                try:
                    cs.plan = ts._new_plan(graph, [x for x in side if x is not None])
                except _lib.SvsError as e:
                    # "auto" never costs a run: a sequence the plan builder refuses (a node type it cannot replay) is
                    # launched as the graph it is (hipGraphLaunch: same results, slower above ~500 rays)
                    if ts.graph != "auto":
                        raise
                    warnings.warn(f"launch plan refused, this configuration replays its hipGraph instead: {e}")
                    cs.plan = None
                    graph.instantiate()
                    if os.environ.get("SVS_PLAN_DEBUG") == "1":
                        print(f"launch plan refused: {e}", file=sys.stderr)
                if cs.plan is not None and os.environ.get("SVS_PLAN_DEBUG") == "1":
                    print(cs.plan.info, file=sys.stderr)
                    print(cs.plan.describe(), file=sys.stderr)
        if cs.plan is not None:
            cs.plan.run()
        else:
            cs.graph.replay()
        return cs.result
