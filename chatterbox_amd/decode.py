"""The decode runtime the two T3 engines share (T3Engine: Llama backbone, T3TurboEngine: GPT-2 backbone): everything around one token step that is not
numerics -- the sampler arguments, the torch capture of the step, the library's token loop (cbx_*_loop_*), chunked decoding (advance / peek / collect), the
per-request state reset and the replay loop.  An engine supplies the step itself (_forward, _decode_step, _use_c_step, _c_step_desc, _get_state) and states
below, as class attributes, where its behaviour differs from the other backbone's.
"""
import torch

from . import ops

START_SPEECH, STOP_SPEECH = 6561, 6562


class _LoopHandle:
    """Owns a cbx_t3_loop_t / cbx_gpt2_loop_t: destroyed, by the library that created it, with the state / geometry entry that holds it."""

    def __init__(self, h, destroy):
        self.h, self.destroy = h, destroy

    def __del__(self):
        try:
            if self.h:
                self.destroy(self.h)
        except Exception:
            pass


class DecodeRuntime:
    # ---- what differs between the backbones: each of these is behaviour
    _SAMPLER_CFG, _SAMPLER_ORDER = None, None  # cbx_sampler_t.cfg / .order: Llama 1 / 0 (CFG row pairs, the reference's processor order), Turbo 0 / 1
    _C_ENTRY = None                 # dict(step=, create=, run=, destroy=): this backbone's stage-level entry points of include/cbx.h
    _ONE_SHOT_C_LOOP = False        # the one-shot generate() runs its token loop in C (Llama); False: it replays the torch-captured graph, the C loop serves advance() only (Turbo)
    _CAPTURE_THREAD_LOCAL = False   # torch captures the step with capture_error_mode="thread_local" (Llama: see T3Engine); False: torch's default
    _ADVANCE_KEEPS_GRAPH = False    # advance() of a state that already holds a torch-captured graph replays THAT, not the C loop (Llama)
    _ADVANCE_CAPTURES = False       # advance() captures the step on first use when it is not on the C loop (Turbo); False: it never captures (Llama)
    _COLLECT_STRIPS_EOS = False     # collect() returns the tokens without a trailing EOS (Turbo)
    weight_dtype = "fp32"
    # what one token step writes: saved around a capture, whose warm-up run must not leak into the real sequence
    _STEP_STATE = ("seen", "step", "done", "n_generated", "out_tokens", "next_ids", "next_pos_ids", "positions", "ctx_lens", "logits")
    # ... and what the step of a GUARDED request writes besides (T3Engine.generate(guard=)): the guard's buffers in st["guard"], and the sampler's parameters
    _GUARD_STATE = ("p", "mass", "state", "sums", "trace")

    # ------------------------------------------------------------------ packed decode images of the current tune
    def _half_tiles(self):
        return bool(self.tune.get("half_tiles"))

    def _tiles(self):
        """(q/k/v tile width, attention-output / MLP-output projection tile width) of the current tune: 16, 12, 8 or 4 output columns per workgroup."""
        tn = self.tune
        return tn.get("qkv_tc") or 16, tn.get("od_tc") or (8 if self._half_tiles() else 16)

    def _image(self, lw, name, tc):
        """The packed decode image of layer weight `name` for `tc`-column tiles (packed on first use: never inside a stream capture,
        generate() calls _prepare_tune() first)."""
        key = f"{name}_pk" if tc == 16 else f"{name}_pk{tc}"
        if key not in lw:
            lw[key] = ops.pack_gemv_weight(lw[name], half_tile=tc, bf16=self.weight_dtype == "bf16")
        return lw[key]

    # ------------------------------------------------------------------ the sampler: launched (_sample) and as the step descriptor's cbx_sampler_t
    def _sampler_kw(self, st):
        # the sampling parameters are read from device memory (st["samp_dev"], one row per utterance): a request with other settings
        # replays the SAME captured decode graph
        return dict(logits=st["logits"], ld=st["logits"].stride(0), V=self.V, B=st["B"], cfg=self._SAMPLER_CFG, order=self._SAMPLER_ORDER, eos_token=STOP_SPEECH,
                    dev_params=st["samp_dev"], seen=st["seen"], uniforms=st["uniforms"], max_steps=st["max_steps"], step=st["step"],
                    out_tokens=st["out_tokens"], done=st["done"], n_generated=st["n_generated"], next_ids=st["next_ids"],
                    next_pos_ids=st["next_pos_ids"], positions=st["positions"], ctx_lens=st["ctx_lens"])

    def _sample(self, st):
        ops.t3_sample(**self._sampler_kw(st))

    def _sampler_desc(self, st):
        from ._lib import SamplerParams
        sp = SamplerParams()
        for k, v in self._sampler_kw(st).items():
            setattr(sp, k, v.data_ptr() if torch.is_tensor(v) else v)
        return sp

    # ------------------------------------------------------------------ the step and the token loop through the stage-level C entry points
    @staticmethod
    def _drop_c_step(st):
        """Take the C step descriptor and the loop handle captured from it out of the state (both bake the geometry in): (descriptor, handle)."""
        return st.pop("cstep", None), st.pop("cloop", None)

    def _decode_step_c(self, st):
        """The token step through the stage-level C entry point (include/cbx.h): one ctypes call enqueues the launches that _forward + _sample issue one by one."""
        import ctypes
        from ._lib import check, lib
        check(getattr(lib, self._C_ENTRY["step"])(ctypes.byref(self._c_step_desc(st)[0]), ops._stream()), self._C_ENTRY["step"])

    def _c_loop(self, st):
        """The loop handle of this state's current geometry (include/cbx.h: the decode step captured in a hipGraph by the LIBRARY), created on first use as
        st["cloop"]; dropped / cached together with the step descriptor it was captured from (_drop_c_step)."""
        import ctypes
        from ._lib import check, lib
        if "cstep" not in st:  # a handle never outlives the descriptor it was captured from
            st.pop("cloop", None)
        d = self._c_step_desc(st)[0]
        if "cloop" not in st:
            h = ctypes.c_void_p()
            torch.cuda.synchronize()
            check(getattr(lib, self._C_ENTRY["create"])(ctypes.byref(d), ops._stream(), ctypes.byref(h)), self._C_ENTRY["create"])
            st["cloop"] = _LoopHandle(h, getattr(lib, self._C_ENTRY["destroy"]))
        return st["cloop"].h

    def _run_c_loop(self, st, n_steps, poll_every):
        import ctypes
        from ._lib import check, lib
        ran = ctypes.c_int(0)
        check(getattr(lib, self._C_ENTRY["run"])(self._c_loop(st), int(n_steps), int(poll_every), ops._stream(), ctypes.byref(ran)), self._C_ENTRY["run"])
        return int(ran.value)

    def _c_loop_serves(self, st):
        return bool(self.c_loop and self._use_c_step(st) and self.dev.type == "cuda")

    # ------------------------------------------------------------------ the step captured by torch
    @staticmethod
    def _graph_slot(st):
        """(dict, key) under which the torch-captured graph of the state's CURRENT step form lives: st["graph"] for the plain step; a guarded request
        (st["guard_on"], T3Engine.generate(guard=)) replays a step with the guard's launches in it, kept beside the plain one in st["guard_graphs"], one per set of
        heads -- neither evicts the other."""
        g = st.get("guard_on")
        return (st, "graph") if g is None else (st.setdefault("guard_graphs", {}), g["heads"])

    def _step_graph(self, st):
        d, k = self._graph_slot(st)
        return d.get(k)

    @torch.inference_mode()
    def _capture(self, st, thread_local=None):
        """torch-captured graph of one token step, as st["graph"] (a guarded state: _graph_slot)."""
        thread_local = self._CAPTURE_THREAD_LOCAL if thread_local is None else thread_local
        torch.cuda.synchronize()
        saved = [(st[k], st[k].clone()) for k in self._STEP_STATE]
        if st.get("guard_on") is not None:  # the guarded step also writes the guard's buffers and the ban column of the sampler's parameters
            saved += [(st["guard"][k], st["guard"][k].clone()) for k in self._GUARD_STATE] + [(st["samp_dev"], st["samp_dev"].clone())]
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode="thread_local" if thread_local else "global"):
            self._decode_step(st)
        for t, v in saved:
            t.copy_(v)
        d, k = self._graph_slot(st)
        d[k] = gr

    # ------------------------------------------------------------------ one request
    @staticmethod
    def _uniform_rows(uniforms, B, n, what):
        """The caller's sampling draws as (B, >= n) floats (None stays None: the engine draws its own)."""
        if uniforms is None:
            return None
        uniforms = torch.as_tensor(uniforms, dtype=torch.float32)
        assert uniforms.numel() % B == 0 and uniforms.numel() // B >= n, f"uniforms must hold at least {what} draws per utterance"
        return uniforms.view(B, -1)

    def _begin_request(self, st, samp, uniforms, n, generator, seeds=None):
        """Reset the per-request state: sampling parameters (B, 8) into device memory (no graph re-capture when a request changes them), sampler counters,
        the n draws of every utterance -- injected, else row b = columns [0, n) of seeds[b]'s RNG_T3_UNIFORMS stream (cbx_rng_fill_f32: no torch RNG is
        consumed), else from the generator / the global RNG."""
        st["samp_dev"].copy_(samp, non_blocking=True)
        for k in ("seen", "step", "done", "n_generated", "out_tokens"):
            st[k].zero_()
        st["seen"][:, START_SPEECH] = 1  # the first processor call sees ids = [start token]
        if uniforms is not None:
            st["uniforms"].copy_(uniforms[:, :n])
        elif seeds is not None:
            ops.rng_fill(st["uniforms"], ops.rng_keys(seeds, ops.RNG_T3_UNIFORMS, device=st["uniforms"].device), n=n)
        else:
            st["uniforms"].uniform_(generator=generator)

    def _ready_step(self, st, use_graph):
        """Capture what _replay will replay, on first use and BEFORE its timed events: the library's loop handle (returns True: the token loop runs in C) or
        the torch graph."""
        if not use_graph or st["max_steps"] <= 1:
            return False
        if self._ONE_SHOT_C_LOOP and self._c_loop_serves(st):
            self._c_loop(st)
            return True
        if self._step_graph(st) is None:
            self._capture(st)
        return False

    def _replay(self, st, n_steps, poll_every=0, c_loop=False, use_graph=True, step_logits=None, event_tag=None):
        """Enqueue up to `n_steps` token steps; returns how many.  c_loop: one call of the library's token loop; else st["graph"] is replayed where there is
        one (and use_graph), else the step is issued eagerly -- forward and sampler split, the raw logits of every step appended, where step_logits is a list.
        poll_every > 0: the done flags are fetched every poll_every steps (a host synchronisation) and the loop ends once every utterance is done.
        event_tag = (prefill lengths, rows): with time_decode, two HIP events around the loop on its launch stream go to decode_events (bench.py)."""
        ev = None
        if self.time_decode and event_tag is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        ran = 0
        if c_loop and n_steps > 0:
            ran = self._run_c_loop(st, n_steps, poll_every)
        graph = self._step_graph(st) if use_graph else None
        for i in range(1, 1 if c_loop else n_steps + 1):
            ran += 1
            if graph is not None:
                graph.replay()
            elif step_logits is not None:
                self._forward(st)
                step_logits.append(st["logits"].clone())
                self._sample(st)
            else:
                self._decode_step(st)
            if poll_every and i % poll_every == 0 and bool(st["done"].all()):
                break
        if ev is not None:
            ev[1].record()
            self.decode_events.append((ev[0], ev[1], ran, *event_tag))
        return ran

    # ------------------------------------------------------------------ chunked decoding: the handle of generate(async_mode=True)
    @ops.on_device
    def advance(self, handle, n_steps):
        """Enqueue up to `n_steps` further token steps of an async generate() (finished utterances are no-ops inside the sampler).  Returns the number of
        steps enqueued.  No host synchronisation (the C loop runs with poll_every = 0)."""
        st = handle["st"]
        if handle.get("guard") is not None:
            raise ValueError("advance() on a guarded handle: the guard covers one-shot requests (generate(guard=) to the end, or async_mode + collect); round "
                             "streams are not built")
        n = max(0, min(int(n_steps), handle["max_new_tokens"] - handle["next_i"]))
        c_loop = self._c_loop_serves(st) and not (self._ADVANCE_KEEPS_GRAPH and st["graph"] is not None)
        if n and not c_loop and self._ADVANCE_CAPTURES and self.dev.type == "cuda" and st["graph"] is None:
            self._capture(st)
        self._replay(st, n, c_loop=c_loop)
        handle["next_i"] += n
        return n

    @ops.on_device
    def peek(self, handle):
        """Tokens sampled so far, EOS included (synchronises with the launch stream): (list of B 1-D LongTensors, list of B done flags)."""
        st, B = handle["st"], handle["B"]
        # (order matters when the decode is still running on ANOTHER stream -- engine.synthesize_stream(overlap=True): the sampler writes token, count, then
        # the done flag, so a done flag read FIRST implies the count read after it is final; a count that is still growing just means "not final yet")
        done = st["done"].tolist()
        n = st["n_generated"].tolist()
        toks = st["out_tokens"].cpu()
        return [toks[b, : n[b]].clone() for b in range(B)], [bool(d) for d in done]

    @ops.on_device
    def collect(self, handle):
        """The tokens of an (async) generate() call as generate() returns them.  Must run on the stream the call was enqueued on."""
        st, B = handle["st"], handle["B"]
        n = st["n_generated"].tolist()
        toks = st["out_tokens"].cpu()
        strip = lambda t: t[:-1] if self._COLLECT_STRIPS_EOS and len(t) and int(t[-1]) == STOP_SPEECH else t
        return [strip(toks[b, : n[b]]).clone() for b in range(B)]
