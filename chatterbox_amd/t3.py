"""T3 speech-token transformer on MI355X: host-side mirror of `T3.inference` (reference models/t3/t3.py:226-390).

Python only sequences kernel launches; all arithmetic runs in libcbx_hip.so.  One decode step (embedding gather ->
30 x [RMSNorm, fused QKV GEMM, RoPE + KV append, decode attention, O-proj + residual, RMSNorm, gate/up GEMM with
SwiGLU epilogue, down-proj + residual] -> final norm -> speech head -> device sampler) is captured ONCE as a
hipGraph and replayed per token: positions, context lengths, the next token id and the EOS flags live in device
memory, so there is no host synchronisation inside the loop (the reference syncs every token, t3.py:366).

Batching (not in the reference, which is batch-1): utterance b occupies row b (conditional) and row B+b (CFG
unconditional); rows are right-padded to a common prefill length -- causal attention keeps padding invisible and
the decode steps then overwrite it in the KV cache at each row's own position.
"""
import math

import os

import torch

from . import ops, weights
from .decode import START_SPEECH, STOP_SPEECH, DecodeRuntime

START_TEXT, STOP_TEXT = 255, 0


def llama3_rope_tables(max_pos, head_dim=64, theta=500000.0, factor=8.0, low=1.0, high=4.0, orig=8192):
    """cos/sin tables [max_pos][64] for HF rope_type 'llama3' (reference llama_configs.py:22-30)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    wl = 2 * math.pi / inv
    scaled = torch.where(wl > orig / low, inv / factor, inv)
    smooth = (orig / wl - low) / (high - low)
    mid = (1 - smooth) * scaled / factor + smooth * scaled
    is_mid = ~(wl < orig / high) & ~(wl > orig / low)
    inv = torch.where(is_mid, mid, scaled)
    fr = torch.arange(max_pos).float()[:, None] * inv[None, :]
    emb = torch.cat([fr, fr], -1)
    return emb.cos().contiguous(), emb.sin().contiguous()


def per_utterance(value, B, name):
    """A sampling parameter as B floats: a scalar serves every utterance, a sequence must hold exactly B values (ValueError before anything is launched)."""
    if torch.is_tensor(value):
        value = value.reshape(-1).tolist() if value.dim() else float(value)
    if isinstance(value, (list, tuple)):
        if len(value) != B:
            raise ValueError(f"{name}: {len(value)} values for {B} utterances")
        return [float(v) for v in value]
    return [float(value)] * B


def sampler_rows(B, cols):
    """Host image (B, 8) of cbx_sampler_t.dev_params: `cols` = the eight columns {cfg_weight, temperature, min_p, top_p, rep_penalty, top_k, ban_token, ban_from},
    each a scalar or a sequence of B."""
    assert len(cols) == 8
    per = [per_utterance(v, B, n) for n, v in cols]
    return torch.tensor([[c[b] for c in per] for b in range(B)], dtype=torch.float32)


def _slice_param(v, lo, hi):
    if torch.is_tensor(v) and v.dim():
        v = v.reshape(-1).tolist()
    return v[lo:hi] if isinstance(v, (list, tuple)) else v


class VoicePrefixCache:
    """K / V of a voice's conditioning positions at every layer, kept after the first prefill with that voice (round 6; T3Engine: 34 positions, the GPT-2 backbones:
    1 + the prompt tokens).  The prompt of T3.inference / inference_turbo is [conditioning | text | BOS] under a causal mask (t3.py:303-335, 407-423): the conditioning
    positions see only themselves, so their K / V depend on the voice alone.  An entry keeps the conditioning tensors alive and is matched by identity + version
    counter (+ content for host tensors; a device tensor made under inference_mode has no counter: identity alone): a hit means the very tensors the prefix was
    computed from.  No device-side compare: generate() must not synchronise (the throughput schedule enqueues ahead).
    A batch may mix voices (a list of cond dicts): every DISTINCT voice has its own entry, cached ones are pasted by voice index in one launch
    (ops.kv_prefix_paste), missing ones are prefilled once per voice -- never once per row."""
    _PREFIX_KEEP = 4

    @staticmethod
    def _tver(t):
        try:
            return t._version
        except RuntimeError:  # "Inference tensors do not track version counter"
            return -1

    def _voice_prefix(self, conds):
        if not (self.share_prefix and isinstance(conds, dict)):
            return None
        for ent in self._prefix_cache:
            ok = ent["keys"] == sorted(conds)
            for k, v, ver, snap in ent["items"] if ok else ():
                c = conds[k]
                if not torch.is_tensor(v):
                    ok = not torch.is_tensor(c) and c == v
                else:  # the very tensor, unmodified: version counter where the tensor has one (inference tensors do not), content for host tensors (a few KB)
                    ok = c is v and self._tver(c) == ver and (snap is None or torch.equal(c, snap))
                if not ok:
                    break
            if ok:
                return ent
        return None

    def _keep_voice_prefix(self, conds, st, P=34, row=0, keep=0):
        """After a prefill: K / V of positions 0 .. P - 1 of cache row `row` (L, H, P, 64).  keep: entries the current batch needs (never evicted by it)."""
        if not (self.share_prefix and isinstance(conds, dict)):
            return None
        ent = self._voice_prefix(conds)
        if ent is not None:
            return ent
        items = [(k, v, self._tver(v) if torch.is_tensor(v) else None, v.clone() if torch.is_tensor(v) and v.device.type == "cpu" else None)
                 for k, v in sorted(conds.items())]
        ent = dict(keys=sorted(conds), items=items, P=P, k=st["kc"][:, row, :, :P].clone(), v=st["vc"][:, row, :, :P].clone(), ev=None)
        if self.dev.type == "cuda":
            ent["ev"] = torch.cuda.Event()
            ent["ev"].record()
        self._prefix_cache.insert(0, ent)
        del self._prefix_cache[max(self._PREFIX_KEEP, keep):]
        return ent

    @staticmethod
    def _distinct_voices(conds, B):
        """(voices, voice_of): the distinct cond dicts of a batch -- one dict, or a list of B in which the same dict (or dicts of the very same tensors / equal
        scalars) may serve several utterances -- and each utterance's index into them.  Host-side identity only: no device compare, no synchronisation."""
        if isinstance(conds, dict):
            return [conds], [0] * B
        assert len(conds) == B, f"{len(conds)} voices for {B} utterances"
        keys, voices, voice_of = {}, [], []
        for c in conds:
            try:
                key = tuple((k, ("t", id(v), VoicePrefixCache._tver(v)) if torch.is_tensor(v) else ("s", v)) for k, v in sorted(c.items()))
                hash(key)
            except TypeError:
                key = ("d", id(c))
            if key not in keys:
                keys[key] = len(voices)
                voices.append(c)
            voice_of.append(keys[key])
        return voices, voice_of

    def _paste_voice_prefixes(self, ents, voice_of_row, st):
        """The cached prefixes of a batch into rows 0 .. len(voice_of_row) - 1 of the KV cache in one launch (ops.kv_prefix_paste); entries may have been written on
        another stream (two decode chains of the throughput schedule)."""
        if self.dev.type == "cuda":
            cur = torch.cuda.current_stream()
            for e in ents:
                if e["ev"] is not None:
                    cur.wait_event(e["ev"])
                    e["k"].record_stream(cur), e["v"].record_stream(cur)
        ops.kv_prefix_paste([(e["k"], e["v"]) for e in ents], voice_of_row, st["kc"], st["vc"])
        # a batch of more than _PREFIX_KEEP voices grew the cache for its own duration (74 MB per voice for Turbo): back to the cap; the pasted entries stay alive
        # in `ents` until the caller returns, and their memory is reused in stream order
        del self._prefix_cache[self._PREFIX_KEEP:]


class T3Engine(DecodeRuntime, VoicePrefixCache):
    D, H, HD, F = 1024, 16, 64, 4096
    # ---- the decode runtime of this backbone (decode.py).  Rows: utterance b is row b (conditional) and row B + b (CFG unconditional), rows = 2 B; a state is
    # keyed by (B, max_ctx, max_steps, slot).
    _SAMPLER_CFG, _SAMPLER_ORDER = 1, 0
    _C_ENTRY = dict(step="cbx_t3_decode_step", create="cbx_t3_loop_create", run="cbx_t3_loop_run", destroy="cbx_t3_loop_destroy")
    _ONE_SHOT_C_LOOP = True      # generate() runs its token loop through cbx_t3_loop_run wherever the C step serves the state (_use_c_step)
    # thread_local: a capture on the T3-enqueue thread of synthesize_pipelined must not make the OTHER host thread's allocations / launches
    # (flow + vocoder of the previous batch, on their own stream) illegal
    _CAPTURE_THREAD_LOCAL = True
    _ADVANCE_KEEPS_GRAPH = True  # advance() takes the C loop only while the state holds no torch-captured graph, and never captures one itself
    MAX_BATCH = 32  # utterances per device batch: 2 CFG rows each, decode GEMV serves M <= 64 rows
    # decode launch geometry: waves per 16-column tile (nw) / cross-workgroup K splits; *2 = the packed-operand (v2) path
    # qkv_tc / od_tc: output columns per workgroup of the q/k/v resp. the o / down projections (0: 16 resp. what half_tiles says; 12 puts
    # q/k/v, 4 puts o / down on exactly 256 workgroups -- with od_tc = 4 and d_ks2 = 1 the down projection needs no partial images and the
    # next q/k/v GEMV no partial-sum fold).  CBX_T3_TUNE="qkv_tc=12,od_tc=4,d_ks2=1,d_nw2=8" overrides any of these for an A/B.
    # qkv_ks / qkv_ct (ABI v11): the q/k/v projection as qkv_ks split-K partial sums over workgroups of qkv_ct column tiles, folded by the attention
    # launch (a CU then moves 96 KiB instead of 256 per q/k/v launch: profiles/r04_decode_launch_timeline.txt); head_ct: column tiles of the head GEMV
    _TUNE = dict(qkv_nw=8, o_ks=4, gu_nw=8, d_ks=8, head_nw=4, o_nw2=8, d_ks2=2, d_nw2=16, half_tiles=1, qkv_tc=0, od_tc=0, prefill_prec=0, qkv_ks=4, qkv_ct=3,
                 head_ct=2)

    @ops.on_device
    def __init__(self, sd, device="cuda", n_layers=None, max_pos=4608, weight_dtype=None):
        self.dev = torch.device(device)
        if n_layers is None:
            n_layers = 0
            while f"tfmr.layers.{n_layers}.input_layernorm.weight" in sd:
                n_layers += 1
        self.L = n_layers
        d = lambda t: t.float().contiguous().to(self.dev)
        self.layers = []
        for i in range(n_layers):
            p = f"tfmr.layers.{i}."
            self.layers.append(dict(
                ln1=d(sd[p + "input_layernorm.weight"]), ln2=d(sd[p + "post_attention_layernorm.weight"]),
                wqkv=d(torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)),
                wo=d(sd[p + "self_attn.o_proj.weight"]),
                wgu=d(weights.pack_swiglu(sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"])),
                wd=d(sd[p + "mlp.down_proj.weight"])))
        # decode path: the same weights in the lane-ordered packed layout of cbx_gemv_f32 (every wave-level load is 1 KiB contiguous)
        self.decode_mode = os.environ.get("CBX_T3_DECODE", "v2")
        # OPT-IN decode numerics (CBX_T3_WEIGHTS=bf16 / T3Engine(weight_dtype="bf16")): the decode-step weight images are rounded to bf16
        # (half the streamed bytes; activations, accumulation, KV cache and the prefill stay fp32).  Not the parity path: sampled
        # tokens differ from the fp32 reference's; stated bound: first-step logits within 5e-2 (SURVEY.md 8d bf16 mode).
        self.weight_dtype = weight_dtype or os.environ.get("CBX_T3_WEIGHTS", "fp32")
        assert self.weight_dtype in ("fp32", "bf16") and (self.weight_dtype == "fp32" or self.decode_mode == "v2")
        bf = self.weight_dtype == "bf16"
        if self.decode_mode == "v2":
            for i, lw in enumerate(self.layers):
                p = f"tfmr.layers.{i}."
                lw["wqkv_pk"] = ops.pack_gemv_weight(lw["wqkv"], bf16=bf)
                lw["wo_pk"] = ops.pack_gemv_weight(lw["wo"], bf16=bf)
                lw["wgu_pk"] = ops.pack_gemv_weight(d(torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], 0)), swiglu=True, bf16=bf)
                lw["wd_pk"] = ops.pack_gemv_weight(lw["wd"], bf16=bf)
                if self._TUNE.get("half_tiles"):  # 8-column tiles for the two N = 1024 projections (128 instead of 64 output tiles)
                    lw["wo_pk8"] = ops.pack_gemv_weight(lw["wo"], half_tile=True, bf16=bf)
                    lw["wd_pk8"] = ops.pack_gemv_weight(lw["wd"], half_tile=True, bf16=bf)
        self.norm = d(sd["tfmr.norm.weight"])
        self.text_emb, self.speech_emb = d(sd["text_emb.weight"]), d(sd["speech_emb.weight"])
        self.text_pos, self.speech_pos = d(sd["text_pos_emb.emb.weight"]), d(sd["speech_pos_emb.emb.weight"])
        self.head = d(sd["speech_head.weight"])
        self.V = self.head.shape[0]
        self.head_pk = ops.pack_gemv_weight(self.head, bf16=bf) if self.decode_mode == "v2" else None
        c = "cond_enc."
        self.spkr_w, self.spkr_b = d(sd[c + "spkr_enc.weight"]), d(sd[c + "spkr_enc.bias"])
        self.emo_w = d(sd[c + "emotion_adv_fc.weight"].view(-1))
        self.pq = d(sd[c + "perceiver.pre_attention_query"][0])
        self.p_ln = (d(sd[c + "perceiver.attn.norm.weight"]), d(sd[c + "perceiver.attn.norm.bias"]))
        self.p_q = (d(sd[c + "perceiver.attn.to_q.weight"]), d(sd[c + "perceiver.attn.to_q.bias"]))
        self.p_kv = (d(torch.cat([sd[c + "perceiver.attn.to_k.weight"], sd[c + "perceiver.attn.to_v.weight"]], 0)),
                     d(torch.cat([sd[c + "perceiver.attn.to_k.bias"], sd[c + "perceiver.attn.to_v.bias"]], 0)))
        self.p_out = (d(sd[c + "perceiver.attn.proj_out.weight"]), d(sd[c + "perceiver.attn.proj_out.bias"]))
        cos, sin = llama3_rope_tables(max_pos)
        self.cos, self.sin = cos.to(self.dev), sin.to(self.dev)
        self.max_pos = max_pos
        self._state = {}
        # decode launch geometry: waves per 16-column tile (nw) and cross-workgroup K splits of the two down-projections
        self.c_step = os.environ.get("CBX_T3_CSTEP", "1") == "1"  # token step through the stage-level C entry point (same kernels)
        self.c_loop = self.c_step and os.environ.get("CBX_T3_CLOOP", "1") == "1"  # ... and the token loop through cbx_t3_loop_* (the hipGraph captured and replayed in C)
        self.time_decode, self.decode_events = False, []  # (start, end, steps, prefill lengths, rows) per generate() when enabled
        self.tune = self._env_tune()
        self.knobs = self._env_knobs()
        # K / V of a voice's 34 conditioning positions at every layer, kept after the first prefill with that voice (round 6; see _voice_prefix)
        self.share_prefix = os.environ.get("CBX_T3_SHARE_PREFIX", "1") == "1"
        self._prefix_cache = []

    # ------------------------------------------------------------------ packed device layout <-> disk (formats.save_packed / load_packed)
    _PLAIN = ("norm", "text_emb", "speech_emb", "text_pos", "speech_pos", "head", "head_pk", "spkr_w", "spkr_b", "emo_w", "pq", "cos", "sin")
    _PAIRS = ("p_ln", "p_q", "p_kv", "p_out")

    def export_packed(self):
        """Every tensor this engine holds after load-time packing, under flat stable names."""
        t = {f"layers.{i}.{k}": v for i, lw in enumerate(self.layers) for k, v in lw.items()}
        t.update({k: getattr(self, k) for k in self._PLAIN if getattr(self, k) is not None})
        for k in self._PAIRS:
            t[k + ".0"], t[k + ".1"] = getattr(self, k)
        return t

    @classmethod
    def from_packed(cls, t, device="cuda", max_pos=4608):
        """Rebuild the engine from `export_packed()` tensors (e.g. memory-mapped by formats.load_packed): no re-packing, one H2D copy each."""
        self = cls.__new__(cls)
        self.dev = torch.device(device)
        d = lambda v: v.to(self.dev) if v.device != self.dev else v
        n = 0
        while f"layers.{n}.ln1" in t:
            n += 1
        self.L = n
        self.layers = [{k.split(".", 2)[2]: d(v) for k, v in t.items() if k.startswith(f"layers.{i}.")} for i in range(n)]
        for k in self._PLAIN:
            setattr(self, k, d(t[k]) if k in t else None)
        for k in self._PAIRS:
            setattr(self, k, (d(t[k + ".0"]), d(t[k + ".1"])))
        self.V = self.head.shape[0]
        self.decode_mode = "v2" if self.head_pk is not None else "v1"
        self.weight_dtype = "bf16" if (self.head_pk is not None and self.head_pk.dtype == torch.bfloat16) else "fp32"
        self.max_pos = self.cos.shape[0]
        self._state = {}
        self.time_decode, self.decode_events = False, []
        self.c_step = os.environ.get("CBX_T3_CSTEP", "1") == "1"
        self.c_loop = self.c_step and os.environ.get("CBX_T3_CLOOP", "1") == "1"
        self.tune = cls._env_tune()
        self.knobs = cls._env_knobs()
        self.share_prefix, self._prefix_cache = os.environ.get("CBX_T3_SHARE_PREFIX", "1") == "1", []
        return self

    @classmethod
    def _env_tune(cls):
        tune = dict(cls._TUNE)
        for kv in filter(None, os.environ.get("CBX_T3_TUNE", "").split(",")):
            k, v = kv.split("=")
            assert k.strip() in tune, f"CBX_T3_TUNE: unknown knob {k!r} (known: {sorted(tune)})"
            tune[k.strip()] = int(v)
        return tune

    @staticmethod
    def _env_knobs():
        """Per-ENGINE launch knobs of the decode attention / GEMVs (da_pipe, da_u, deep, pre_epi): they travel in every call's descriptor
        (cbx_decode_attn_t, cbx_gemv_t.flags; ABI v10), nothing is process-wide.  Defaults from CBX_DA_PIPE / CBX_DA_U / CBX_GEMV_* (A/B scripts)."""
        from .autotune import env_knobs
        return env_knobs()

    def _gf(self):
        return ops.gemv_flags(self.knobs.get("pre_epi"), self.knobs.get("deep"), self.knobs.get("shallow"))

    def _sync_geom(self, st):
        st["da"].unroll, st["da"].pipeline = (0 if int(self.knobs["da_u"]) == 4 else int(self.knobs["da_u"])), int(self.knobs["da_pipe"])

    def _qks(self):
        """Effective split-K factor of the q/k/v projection (0 = the one-tile kernel): the column-tile form serves the 16-column fp32 image."""
        ks = int(self.tune.get("qkv_ks") or 0)
        return ks if ks > 1 and not self.tune.get("qkv_tc") and self.weight_dtype == "fp32" and self.D % (256 * ks) == 0 else 0

    def _hct(self):
        return int(self.tune.get("head_ct") or 0) if self.weight_dtype == "fp32" and self.D % 256 == 0 else 0

    def _half_tiles(self):
        return bool(self.tune.get("half_tiles")) and "wo_pk8" in self.layers[0]

    def _prepare_tune(self):
        if self.decode_mode != "v2":
            return
        qtc, odtc = self._tiles()
        assert qtc in (16, 12) and odtc in (16, 8, 4), f"tile widths {qtc} / {odtc}"
        tn = self.tune
        assert tn.get("qkv_ks", 0) in (0, 1, 2, 4) and 1 <= tn.get("qkv_ct", 3) <= 4 and 0 <= tn.get("head_ct", 0) <= 4, f"column-tile geometry {tn}"
        # (qkv_tc = 12 or bf16 weight images switch the split-K / column-tile forms off: _qks(), _hct())
        for lw in self.layers:
            self._image(lw, "wqkv", qtc), self._image(lw, "wo", odtc), self._image(lw, "wd", odtc)

    # ------------------------------------------------------------------ decode-step geometry: measured, not guessed (autotune.py)
    def apply_variant(self, tune, knobs=None):
        """Switch the decode geometry of THIS engine: `tune` replaces self.tune, `knobs` (da_pipe, da_u, deep, pre_epi) the launch knobs of the
        decode attention / GEMV load batches -- per-call descriptor fields since ABI v10, so another engine in the process keeps its own.
        Captured decode graphs and C step descriptors bake the geometry in: they are dropped."""
        from .autotune import LIB_KNOBS, canon
        old_key = canon(self.tune, self.knobs) + (("shallow", int(bool(self.knobs.get("shallow")))),)
        self.tune = dict(tune)
        self.knobs = dict(LIB_KNOBS, **(knobs or {}))
        assert int(self.knobs["da_pipe"]) in range(8) and int(self.knobs["da_u"]) in (4, 8, 16)
        new_key = canon(self.tune, self.knobs) + (("shallow", int(bool(self.knobs.get("shallow")))),)
        for st in self._state.values():
            # the captured graph / C step descriptor of a state are kept PER GEOMETRY (alternating synthesize() and synthesize_pipelined()
            # re-captured the decode graph on every switch); they reference the state's own buffers and the weight images, which both outlive the switch
            cache = st.setdefault("geom_cache", {})
            cache[old_key] = {k: st.pop(k) for k in ("graph", "cstep", "cloop", "guard_graphs") if k in st}
            st["graph"] = None
            st.update(cache.pop(new_key, {}))
            self._sync_geom(st)
        if getattr(self, "_co_res", False) and not getattr(self, "_co_switching", False):
            # a geometry adopted WHILE the co-resident form is on becomes the one co_resident(False) returns to (its co-resident keys aside)
            self._co_saved = (dict(self._co_saved[0], **{k: v for k, v in self.tune.items() if k not in ("half_tiles", "d_ks2", "d_nw2")}),
                              dict(self._co_saved[1], **{k: v for k, v in self.knobs.items() if k != "shallow"}))

    def co_resident(self, on):
        """The decode step on the geometry whose workgroups fit on a CU BESIDE a co-resident flow workgroup (engine.synthesize_pipelined; profiles/r05_overlap_*):
        every launch <= 8 waves x <= 128 VGPRs -- the down projection on 512-thread workgroups with 4 split-K partial images (a member of the hardware-green
        allow-list: decode_green.json {d_ks2: 4, d_nw2: 8, half_tiles: 0}), gate | up on its 2-deep load batches (CBX_GEMV_SHALLOW: same products, same order).
        on=False: back to the engine's default geometry.  Switching drops the captured decode graphs."""
        if getattr(self, "_co_res", False) == bool(on):
            return
        self._co_switching = True
        try:
            if on:
                self._co_saved = (dict(self.tune), dict(self.knobs))
                self.apply_variant(dict(self.tune, half_tiles=0, d_ks2=4, d_nw2=8), dict(self.knobs, shallow=1))
            else:
                self.apply_variant(*self._co_saved)
        finally:
            self._co_switching = False
        self._co_res = bool(on)

    @ops.on_device
    @torch.inference_mode()
    def measure_decode(self, B=8, ctx=224, steps=24, reps=2, use_graph=True, slot=7, two_tile=False):
        """(ms per token step, logits after ONE step) of the current geometry on a seeded synthetic decode state: 2 B rows that hold `ctx`
        cached positions each.  The step is the one generate() replays (embedding .. sampler, one hipGraph); time = HIP events around
        `steps` replays, best of `reps`.  The logits are a pure function of the seed, so two geometries can be compared bit for bit.
        two_tile: 17 .. 32 rows on the packed five-launch layer (generate(two_tile=True))."""
        import time
        rows = 2 * B
        total = 4 + reps * steps
        max_ctx = (ctx + total + 1 + 63) // 64 * 64
        assert max_ctx <= self.max_pos
        st = self._get_state(B, max_ctx, total + 1, slot)
        self._prepare_tune()
        st["graph"] = None
        self._drop_c_step(st)
        st.pop("geom_cache", None)
        st["two_tile"] = bool(two_tile)
        gen = torch.Generator(device=self.dev).manual_seed(20240229)
        for k in ("kc", "vc"):
            st[k].normal_(0.0, 0.5, generator=gen)
        st["uniforms"].uniform_(generator=gen)
        for k in ("seen", "step", "done", "n_generated", "out_tokens"):
            st[k].zero_()
        st["samp_dev"].copy_(torch.tensor([0.5, 0.8, 0.05, 1.0, 1.2, 0.0, float(STOP_SPEECH), 6561.0]).repeat(B, 1))
        ids = torch.tensor([(911 * b + 17) % 6561 for b in range(B)] * 2, dtype=torch.int64)
        st["next_ids"].copy_(ids)
        st["next_pos_ids"].fill_(1)
        st["positions"].fill_(ctx)
        st["ctx_lens"].fill_(ctx + 1)
        self._decode_step(st)
        logits = st["logits"].clone()
        if steps <= 0:  # numerics only
            return 0.0, logits
        cuda = self.dev.type == "cuda"
        if cuda and use_graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._decode_step(st)
            step = g.replay
        else:
            step = lambda: self._decode_step(st)
        step()
        best = float("inf")
        for _ in range(reps):
            if cuda:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    step()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1)
            else:
                t0 = time.perf_counter()
                for _ in range(steps):
                    step()
                ms = 1e3 * (time.perf_counter() - t0)
            best = min(best, ms / steps)
        if cuda:
            torch.cuda.synchronize()
        # the state the whole run ended in (a pure function of the seed and of the arithmetic)
        self.last_measure = dict(final_logits=st["logits"].clone(), out_tokens=st["out_tokens"].clone())
        st["graph"] = None
        self._drop_c_step(st)
        return best, logits

    @ops.on_device
    @torch.inference_mode()
    def probe_decode(self, B=8, ctxs=(1, 38, 63, 64, 65, 225, 640), slot=7):
        """Logits of ONE token step per entry of `ctxs` on a seeded synthetic state whose rows hold RAGGED contexts (row r: (c - 1 + 37 r) mod
        704 cached positions): what two geometries that claim the same arithmetic must agree on bit for bit.  The autotuner's identity check
        (one step at the bench context never looked at contexts shorter than one 64-position attention step, or at the split grid)."""
        rows, max_ctx = 2 * B, 704
        st = self._get_state(B, max_ctx, 4, slot)
        self._prepare_tune()
        st["graph"] = None
        self._drop_c_step(st)
        gen = torch.Generator(device=self.dev).manual_seed(20250922)
        for k in ("kc", "vc"):
            st[k].normal_(0.0, 0.5, generator=gen)
        st["uniforms"].uniform_(generator=gen)
        st["samp_dev"].copy_(torch.tensor([0.5, 0.8, 0.05, 1.0, 1.2, 0.0, float(STOP_SPEECH), 6561.0]).repeat(B, 1))
        ids = torch.tensor([(911 * b + 17) % 6561 for b in range(B)] * 2, dtype=torch.int64)
        out = []
        for c in ctxs:
            for k in ("seen", "step", "done", "n_generated", "out_tokens"):
                st[k].zero_()
            pos = torch.tensor([(c - 1 + 37 * r) % (max_ctx - 8) for r in range(rows)], dtype=torch.int32)
            st["next_ids"].copy_(ids)
            st["next_pos_ids"].fill_(1)
            st["positions"].copy_(pos)
            st["ctx_lens"].copy_(pos + 1)
            self._decode_step(st)
            out.append(st["logits"].clone())
        return torch.stack(out)

    def autotune(self, B=8, ctx=224, steps=24, reps=2, min_gain=0.01, allow_reorder=False, in_child=True, timeout=180.0, log=None, tiles=None, attn=None,
                 epi=None, validate=None, green_only=False):
        """Measure the decode-step geometries (autotune.py) and adopt the fastest one whose logits are bit-identical to the current
        geometry's.  in_child: the candidates run in a child process on synthetic weights of this shape, so a faulting candidate cannot take
        the serving process down; its failure leaves the geometry unchanged.  validate: a callable run on THIS engine after the fastest
        candidate overall -- possibly one that sums the down projection in another fp32 order -- has been applied; it is kept only if the
        callable returns True (e.g. "the serving workload's tokens are the ones the built-in geometry samples"), otherwise the bit-identical
        winner is.  Returns the report (also kept as self.autotune_report)."""
        from . import autotune as at
        knobs = dict(self.knobs)
        tune0 = dict(self.tune)
        if self.decode_mode != "v2" or 2 * B > 16:
            rep = dict(best={}, skipped="the tile / pipeline variants serve the packed <= 16-row decode path")
        elif in_child:
            base = {k: v for k, v in self.tune.items() if v != self._TUNE.get(k)}
            rep = at.tune_in_child(self.L, B, ctx, steps, reps, min_gain, allow_reorder, self.dev.index or 0, base, knobs, timeout, log, green_only=green_only)
        else:
            rep = at.tune_decode(self, B, ctx, steps, reps, min_gain, allow_reorder, use_graph=self.dev.type == "cuda", log=log,
                                 tiles=tiles or at.TILE_VARIANTS, attn=at.ATTN_VARIANTS if attn is None else attn,
                                 epi=at.EPI_VARIANTS if epi is None else epi, green_only=green_only)

        def adopt(v):
            t, k = at.split_variant(v)
            self.apply_variant(dict(tune0, **t), dict(knobs, **k))
            with torch.inference_mode():
                self._prepare_tune()

        best, best_any = rep.get("best") or {}, rep.get("best_any") or {}
        adopted = best
        if validate is not None and best_any and best_any != best:
            adopt(best_any)
            try:
                ok = bool(validate())
            except Exception as e:
                ok = False
                rep["validate_error"] = f"{type(e).__name__}: {e}"[:200]
            rep["best_any_validated"] = ok
            if ok:
                adopted = best_any
        if adopted or (validate is not None and best_any and best_any != best):
            adopt(adopted)
        rep["adopted"] = adopted
        for key in [k for k in self._state if k[3] == 7]:  # the measurement's own state (KV cache of the synthetic context)
            del self._state[key]
        self.autotune_report = rep
        return rep

    # ------------------------------------------------------------------ conditioning (t3.py:92-100, cond_enc.py:64-97)
    def _perceiver_block(self, x1, x2):
        """AttentionBlock2.forward (perceiver.py:156-170): x1 (n1,1024) queries attend to x2 (n2,1024)."""
        f = lambda *s: torch.empty(*s, device=self.dev)
        n1, n2 = x1.shape[0], x2.shape[0]
        h1, h2 = f(n1, 1024), f(n2, 1024)
        ops.layernorm(x1, self.p_ln[0], self.p_ln[1], h1)
        ops.layernorm(x2, self.p_ln[0], self.p_ln[1], h2)
        q, kv = f(n1, 1024), f(n2, 2048)
        ops.linear(h1, self.p_q[0], q, bias=self.p_q[1])
        ops.linear(h2, self.p_kv[0], kv, bias=self.p_kv[1])
        n2p = (n2 + 3) // 4 * 4
        s, pr = f(1, 4, n1, n2p), f(1, 4, n1, n2p)
        kv8 = kv.view(1, n2, 8, 256)  # heads 0-3 = K heads, 4-7 = V heads
        ops.bmm(q.view(1, n1, 4, 256).permute(0, 2, 1, 3), kv8[:, :, :4].permute(0, 2, 1, 3), s[..., :n2])
        ops.softmax_rows(s, pr, 1.0 / 16.0, n2)
        o = f(n1, 1024)
        ops.bmm(pr[..., :n2], kv8[:, :, 4:].permute(0, 2, 1, 3), o.view(1, n1, 4, 256).permute(0, 2, 1, 3), nn=True)
        out = f(n1, 1024)
        ops.linear(o, self.p_out[0], out, bias=self.p_out[1], residual=x1)
        return out

    @ops.on_device
    def cond_embeds(self, cond):
        """T3.prepare_conditioning -> (34, 1024): [speaker | 32 perceiver latents | emotion]."""
        dev = self.dev
        out = torch.empty(34, 1024, device=dev)
        spk = cond["speaker_emb"].to(dev).float().view(1, 256)
        ops.linear(spk, self.spkr_w, out[0:1], bias=self.spkr_b)
        toks = cond["cond_prompt_speech_tokens"].to(dev).long().view(-1)
        n = toks.shape[0]
        pe = torch.empty(n, 1024, device=dev)
        ops.embed(toks, self.speech_emb, pe, table2=self.speech_pos, ids2=torch.arange(n, dtype=torch.int32, device=dev))
        pre = self._perceiver_block(self.pq, pe)
        out[1:33] = self._perceiver_block(pre, pre)
        emo = float(torch.as_tensor(cond["emotion_adv"]).reshape(-1)[0])
        ops.axpby(self.emo_w.view(1, -1), out[33:34], a=emo, b=0.0)
        return out

    # ------------------------------------------------------------------ the conditioning prefix of a voice (round 6: VoicePrefixCache)
    # Later prefills with the SAME conditioning tensors run over the text positions only (a third fewer rows in every prefill GEMM at 64 text tokens) and read the
    # prefix keys from the cache (cbx_flash_attn_kv_f32).
    def _layer_prefill_text(self, lw, x, ws, St, S, rows, kc, vc, pos, crow, after_rope=None):
        """_layer_prefill over the text positions alone: queries from the q | k | v workspace, keys / values [cached prefix | text] from the KV cache.
        after_rope(q4, kc): called once the layer's rotated q is in the workspace and its k in the cache (the alignment pass reads both there)."""
        ops.layernorm(x, lw["ln1"], None, ws["h"], 1e-5, rms=True)
        ops.linear(ws["h"], lw["wqkv"], ws["qkv"])
        ops.rope_kv(ws["qkv"], pos, self.cos, self.sin, kc, vc, self.H, cache_rows=crow)
        q4 = ws["qkv"].view(rows, St, 3, self.H, 64)
        if after_rope is not None:
            after_rope(q4, kc)
        ops.flash_attn(q4[:, :, 0], kc[:rows, :, :S].permute(0, 2, 1, 3), vc[:rows, :, :S].permute(0, 2, 1, 3), ws["att"].view(rows, St, self.H, 64), 0.125,
                       causal=True)
        ops.linear(ws["att"], lw["wo"], x, residual=x)
        ops.layernorm(x, lw["ln2"], None, ws["h"], 1e-5, rms=True)
        ops.linear(ws["h"], lw["wgu"], ws["g"], swiglu=True)
        ops.linear(ws["g"], lw["wd"], x, residual=x)

    # ------------------------------------------------------------------ one transformer layer
    def _layer_prefill(self, lw, x, ws, S, rows, kc, vc, pos, crow):
        M = rows * S
        ops.layernorm(x, lw["ln1"], None, ws["h"], 1e-5, rms=True)
        ops.linear(ws["h"], lw["wqkv"], ws["qkv"])
        ops.rope_kv(ws["qkv"], pos, self.cos, self.sin, kc, vc, self.H, cache_rows=crow)
        q4 = ws["qkv"].view(rows, S, 3, self.H, 64)
        ops.flash_attn(q4[:, :, 0], q4[:, :, 1], q4[:, :, 2], ws["att"].view(rows, S, self.H, 64), 0.125, causal=True)
        ops.linear(ws["att"], lw["wo"], x, residual=x)
        ops.layernorm(x, lw["ln2"], None, ws["h"], 1e-5, rms=True)
        ops.linear(ws["h"], lw["wgu"], ws["g"], swiglu=True)
        ops.linear(ws["g"], lw["wd"], x, residual=x)

    def _prefill_rows(self, xf, S, rows, st, pos, crow, prec, pws=None):
        """The full prefill of `rows` rows of S positions each (xf (rows * S, D) in / out): through cbx_t3_prefill, or launch by launch under a kernel timer."""
        dev = self.dev
        if pws is None:
            pws = dict(h=torch.empty(rows * S, self.D, device=dev), qkv=torch.empty(rows * S, 3 * self.D, device=dev),
                       att=torch.empty(rows * S, self.D, device=dev), g=torch.empty(rows * S, self.F, device=dev))
        if self.c_step and not ops.TIMER:  # the same launches through the stage-level C entry point cbx_t3_prefill (one ctypes call instead of 9 per layer)
            self._prefill_c(xf, pws, S, rows, st, pos, crow)
        else:
            with ops.gemm_precision(prec):
                for i, lw in enumerate(self.layers):
                    self._layer_prefill(lw, xf, pws, S, rows, st["kc"][i], st["vc"][i], pos, crow)

    def _layer_array(self, decode=False):
        """A fresh cbx_t3_layer_t[L] of the row-major weights the prefill reads, or (decode) of the packed decode images of the current tile widths."""
        from ._lib import T3Layer
        arr = (T3Layer * self.L)()
        qtc, odtc = self._tiles()
        for i, lw in enumerate(self.layers):
            ws = (self._image(lw, "wqkv", qtc), self._image(lw, "wo", odtc), lw["wgu_pk"], self._image(lw, "wd", odtc)) if decode else \
                (lw["wqkv"], lw["wo"], lw["wgu"], lw["wd"])
            arr[i].ln1, arr[i].ln2 = lw["ln1"].data_ptr(), lw["ln2"].data_ptr()
            arr[i].wqkv, arr[i].wo, arr[i].wgu, arr[i].wd = (w.data_ptr() for w in ws)
        return arr

    def _prefill_c(self, xf, ws, S, rows, st, pos, crow):
        """The prefill through cbx_t3_prefill (include/cbx.h): the launches of _layer_prefill x n_layers, sequenced in C."""
        import ctypes
        from ._lib import T3Prefill, check, lib
        p = lambda t: t.data_ptr()
        arr = self._layer_array()  # built per call (30 x 6 pointers): a cached array would outlive a re-packed / re-loaded weight tensor
        d = T3Prefill()
        d.n_layers, d.rows, d.S, d.dim, d.ffn, d.n_heads, d.precision = self.L, rows, S, self.D, self.F, self.H, int(self.tune.get("prefill_prec") or 0)
        d.eps, d.attn_scale, d.layers = 1e-5, 0.125, arr
        d.x, d.h, d.qkv, d.att, d.g = p(xf), p(ws["h"]), p(ws["qkv"]), p(ws["att"]), p(ws["g"])
        d.positions, d.cache_rows, d.cos_t, d.sin_t, d.kc, d.vc = p(pos), p(crow), p(self.cos), p(self.sin), p(st["kc"]), p(st["vc"])
        d.kv_layer_stride, d.kv_row_stride, d.kv_head_stride = st["kc"].stride(0), st["kc"].stride(1), st["kc"].stride(2)
        check(lib.cbx_t3_prefill(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "cbx_t3_prefill")

    def _forward_decode(self, st):
        """One token for every row.  The residual stream x is only touched by add_rmsnorm, which folds the split-K
        partials of the previous projection, the residual add and the RMSNorm into one pass."""
        ws, x, tn = st["dws"], st["dws"]["x"], self.tune
        h, qkv, att, g, po, pd = ws["h"], ws["qkv"], ws["att"], ws["g"], ws["po"][: tn["o_ks"]], ws["pd"][: tn["d_ks"]]
        ops.embed(st["next_ids"], self.speech_emb, x, table2=self.speech_pos, ids2=st["next_pos_ids"])
        part = None
        for i, lw in enumerate(self.layers):
            ops.add_rmsnorm(x, part, lw["ln1"], h)
            ops.gemv(h, lw["wqkv"], qkv, nw=tn["qkv_nw"])
            ops.decode_attn_rope(qkv, st["positions"], self.cos, self.sin, st["kc"][i], st["vc"][i], att, 0.125, geom=st["da"])
            if st.get("guard_on") is not None:
                self._guard_mass(st, i, qkv)
            ops.gemv(att, lw["wo"], po, ksplit=tn["o_ks"], nw=4)
            ops.add_rmsnorm(x, po, lw["ln2"], h)
            ops.gemv(h, lw["wgu"], g, swiglu=True, nw=tn["gu_nw"])
            ops.gemv(g, lw["wd"], pd, ksplit=tn["d_ks"], nw=4)
            part = pd
        ops.add_rmsnorm(x, part, self.norm, h)
        ops.gemv(h, self.head, st["logits"], nw=tn["head_nw"])

    def _forward_decode_v2(self, st):
        """5 launches per layer and no standalone norm / reduce kernels.  Every GEMV operand lives in the lane-ordered packed layout
        (written that way by its producer); RMSNorm is folded into the q/k/v, gate/up and head GEMVs (x * norm_w on the way to the
        MFMA, rstd in the epilogue); the o projection (4 MB) adds the residual in its epilogue; the down projection (16.8 MB, needs all
        256 CUs) emits `d_ks` split-K partial images that the NEXT consumer (q/k/v of the following layer, or the head) sums into its x
        operand on the fly, writing the new residual stream to the other ping-pong image."""
        ws, tn = st["dws"], self.tune
        rows, dks = st["rows"], tn["d_ks2"]
        cur, nxt, qkv, att, g, pd = ws["x_pk"], ws["x2_pk"], ws["qkv"], ws["att_pk"], ws["g_pk"], ws["pd_pk"][:dks]
        pk = dict(w_packed=True, x_packed=True, M=rows, flags=self._gf())
        ops.embed(st["next_ids"], self.speech_emb, cur, table2=self.speech_pos, ids2=st["next_pos_ids"], out_packed=True)
        red = {}  # partial images pending on the residual stream
        qtc, odtc = self._tiles()
        qt, ot = (0 if qtc == 16 else qtc), (0 if odtc == 16 else odtc)
        qks, qct, hct = self._qks(), int(tn.get("qkv_ct") or 3), self._hct()
        for i, lw in enumerate(self.layers):
            if qks > 1:  # split-K partial sums over column-tile workgroups; the attention launch adds them and applies rstd (ABI v11)
                qp, sq = ws["qkv_parts"][:qks], ws["qkv_ssq"][:qks]
                ops.gemv(cur, lw["wqkv_pk"], qp, N=3 * self.D, K=self.D, nw=8, norm_w=lw["ln1"], col_tiles=qct, ksplit=qks, ssq_out=sq, **pk, **red)
            else:
                ops.gemv(cur, self._image(lw, "wqkv", qtc), qkv, N=3 * self.D, K=self.D, nw=8, norm_w=lw["ln1"], half_tile=qt, **pk, **red)
            if red:
                cur, nxt = nxt, cur  # the q/k/v GEMV wrote x + sum(partials) to the other image
            if qks > 1:
                ops.decode_attn_rope(qp, st["positions"], self.cos, self.sin, st["kc"][i], st["vc"][i], att, 0.125, out_packed=True, geom=st["da"],
                                     qkv_ssq=sq, rms_dim=self.D, rms_eps=1e-5)
            else:
                ops.decode_attn_rope(qkv, st["positions"], self.cos, self.sin, st["kc"][i], st["vc"][i], att, 0.125, out_packed=True, geom=st["da"])
            if st.get("guard_on") is not None:  # the alignment guard reads the same q and this layer's K, the new position included
                self._guard_mass(st, i, qp if qks > 1 else qkv, sq if qks > 1 else None)
            ops.gemv(att, self._image(lw, "wo", odtc), cur, N=self.D, K=self.D, nw=tn["o_nw2"], res=cur, out_packed=True, half_tile=ot, **pk)
            ops.gemv(cur, lw["wgu_pk"], g, N=self.F, K=self.D, swiglu=True, nw=tn["gu_nw"], norm_w=lw["ln2"], out_packed=True, **pk)
            if dks > 1:
                ops.gemv(g, self._image(lw, "wd", odtc), pd, N=self.D, K=self.F, ksplit=dks, nw=tn["d_nw2"], out_packed=True, half_tile=ot, **pk)
                red = dict(xpart=pd, x_out=nxt)
            else:  # the down projection adds the residual itself: no partial images, no fold in the next q/k/v GEMV
                ops.gemv(g, self._image(lw, "wd", odtc), cur, N=self.D, K=self.F, nw=tn["d_nw2"], res=cur, out_packed=True, half_tile=ot, **pk)
        if red:
            red["x_out"] = None
        ops.gemv(cur, self.head_pk, st["logits"], N=self.V, K=self.D, nw=8, norm_w=self.norm, col_tiles=hct, **red, **pk)

    def _packed_rows(self, st):
        """Does this state's token step run on the packed five-launch layer?  Up to 16 rows always.  17 .. 32 rows (two row tiles: every launch streams its weights
        once for both tiles, each row bit for bit what its 16-row launch gives -- csrc/gemv_decode.hip) where the state asks for it (generate(two_tile=True): the
        paired batches of engine.synthesize_pipelined), on fp32 images, with at most 3 column tiles per workgroup, unguarded (the guard's launches read 16-row
        q/k/v partial sums).  33 .. 64 rows, and 17 .. 32 without the switch: the 9-launch step (DESIGN.md section 4 has both measured)."""
        if self.decode_mode != "v2":
            return False
        if st["rows"] <= 16:
            return True
        return bool(st.get("two_tile")) and st["rows"] <= 32 and self.weight_dtype == "fp32" and st.get("guard_on") is None \
            and int(self.tune.get("qkv_ct") or 3) <= 3 and self._hct() <= 3 and not self.tune.get("qkv_tc")

    def _forward(self, st):
        if self._packed_rows(st):
            self._forward_decode_v2(st)
        else:
            self._forward_decode(st)
        if st.get("guard_on") is not None:  # between the head GEMV and the sampler
            self._guard_update(st)

    def _decode_step(self, st):
        if self._use_c_step(st):
            return self._decode_step_c(st)
        self._forward(st)
        self._sample(st)

    def _use_c_step(self, st):
        # (a guarded request takes the Python-sequenced step: the C step has no descriptor for the guard's launches)
        return self.c_step and self._packed_rows(st) and self.tune["d_ks2"] in (1, 2, 4) and st.get("guard_on") is None

    def _c_step_desc(self, st):
        """Build (once per state and geometry) the cbx_t3_step_t of this state: st["cstep"] = (descriptor, layers, sampler).  One call of it enqueues the
        153 launches that _forward_decode_v2 + _sample issue one by one."""
        import ctypes
        from ._lib import T3Step
        if "cstep" not in st:
            p = lambda t: t.data_ptr()
            ws, tn = st["dws"], self.tune
            qtc, odtc = self._tiles()
            layers, sp = self._layer_array(decode=True), self._sampler_desc(st)
            d = T3Step()
            d.n_layers, d.rows, d.dim, d.ffn, d.n_heads, d.vocab = self.L, st["rows"], self.D, self.F, self.H, self.V
            d.o_nw, d.gu_nw, d.d_nw, d.d_ksplit, d.eps, d.attn_scale = tn["o_nw2"], tn["gu_nw"], tn["d_nw2"], tn["d_ks2"], 1e-5, 0.125
            d.half_tiles, d.qkv_tile = (0 if odtc == 16 else odtc), (0 if qtc == 16 else qtc)
            d.w_bf16 = int(self.head_pk.dtype == torch.bfloat16)
            d.layers = layers
            d.speech_emb, d.speech_pos, d.final_norm, d.head = p(self.speech_emb), p(self.speech_pos), p(self.norm), p(self.head_pk)
            d.cos_t, d.sin_t, d.kc, d.vc = p(self.cos), p(self.sin), p(st["kc"]), p(st["vc"])
            d.kv_row_stride, d.kv_head_stride = st["kc"].stride(1), st["kc"].stride(2)
            d.next_ids, d.next_pos_ids, d.positions = p(st["next_ids"]), p(st["next_pos_ids"]), p(st["positions"])
            d.x_a, d.x_b, d.qkv, d.att, d.g, d.pd = p(ws["x_pk"]), p(ws["x2_pk"]), p(ws["qkv"]), p(ws["att_pk"]), p(ws["g_pk"]), p(ws["pd_pk"])
            d.logits, d.ld_logits, d.sampler = p(st["logits"]), st["logits"].stride(0), ctypes.pointer(sp)
            da = st["da"]  # the step's own attention geometry + split-context workspace, GEMV flags (ABI v10: nothing process-wide)
            d.da_unroll, d.da_pipeline, d.da_split_min, d.gemv_flags = da.unroll, da.pipeline, da.split_min, self._gf()
            qks = self._qks()
            if qks > 1:
                d.qkv, d.qkv_ksplit, d.qkv_ct, d.qkv_ssq = p(ws["qkv_parts"]), qks, int(tn.get("qkv_ct") or 3), p(ws["qkv_ssq"])
            d.head_ct = self._hct()
            d.da_ws, d.da_cnt, d.da_pairs = ops._p(da.ws), ops._p(da.cnt), (da.max_pairs if da.ws is not None else 0)  # None: >= 128 (row, head) pairs never split
            st["cstep"] = (d, layers, sp)  # keep the host structures alive
        return st["cstep"]

    # ------------------------------------------------------------------ state / workspaces
    def release_state(self, slot):
        """Drop every decode state (KV cache, workspaces, captured graph) of `slot`: measure_decode / probe_decode park theirs in slot 7
        (≈ 2.6 GB at B = 8, L = 30), which a serving engine must get back after an in-process autotune."""
        for k in [k for k in self._state if k[3] == slot]:
            del self._state[k]

    def _get_state(self, B, max_ctx, max_steps, slot=0):
        key = (B, max_ctx, max_steps, slot)
        if key in self._state:
            # whoever takes the state starts unguarded: generate() sets the flag for ITS request right after; measure_decode / probe_decode never do
            self._state[key]["guard_on"] = None
            return self._state[key]
        for k in [k for k in self._state if k[3] == slot]:  # one live configuration per slot (the KV cache dominates memory)
            del self._state[k]
        dev, rows = self.dev, 2 * B
        f = lambda *s: torch.empty(*s, device=dev)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        st = dict(B=B, rows=rows, max_ctx=max_ctx, max_steps=max_steps,
                  kc=torch.zeros(self.L, rows, self.H, max_ctx, 64, device=dev),
                  vc=torch.zeros(self.L, rows, self.H, max_ctx, 64, device=dev),
                  logits=f(rows, self.V), seen=torch.zeros(B, self.V, dtype=torch.uint8, device=dev),
                  uniforms=f(B, max_steps), step=i32(B), out_tokens=torch.zeros(B, max_steps, dtype=torch.int64, device=dev),
                  done=i32(B), n_generated=i32(B), next_ids=torch.zeros(rows, dtype=torch.int64, device=dev),
                  next_pos_ids=i32(rows), positions=i32(rows), ctx_lens=i32(rows),
                  dws=dict(x=f(rows, self.D), h=f(rows, self.D), qkv=f(rows, 3 * self.D), att=f(rows, self.D), g=f(rows, self.F),
                           po=f(8, rows, self.D), pd=f(8, rows, self.D),
                           # packed operand images of the v2 decode path (rows padded to whole 16-row tiles, pad rows stay 0)
                           x_pk=torch.zeros((rows + 15) // 16 * 16, self.D, device=dev),
                           att_pk=torch.zeros((rows + 15) // 16 * 16, self.D, device=dev),
                           x2_pk=torch.zeros((rows + 15) // 16 * 16, self.D, device=dev),
                           pd_pk=torch.zeros(4, (rows + 15) // 16 * 16, self.D, device=dev),
                           g_pk=torch.zeros((rows + 15) // 16 * 16, self.F, device=dev),
                           # split-K partial sums of the q/k/v projection + their sums of squares (tune qkv_ks, ABI v11)
                           qkv_parts=torch.zeros(4, rows, 3 * self.D, device=dev), qkv_ssq=torch.zeros(4, (rows + 15) // 16 * 16 if rows <= 32 else 16, device=dev)),
                  graph=None, samp_dev=torch.zeros(B, 8, device=dev),
                  # geometry + split-context workspace of this state's attention launches (a state = one stream of launches; two slots may be in flight)
                  da=ops.DecodeAttnGeom(dev, split=rows * self.H < 128))
        self._sync_geom(st)
        self._state[key] = st
        return st

    # ------------------------------------------------------------------ T3.inference
    @ops.on_device
    @torch.inference_mode()
    def generate(self, conds, text_tokens, max_new_tokens=1000, temperature=0.8, top_p=1.0, min_p=0.05,
                 repetition_penalty=1.2, cfg_weight=0.5, uniforms=None, ban_eos=False, ban_from=0, use_graph=True, poll_every=16,
                 return_prefill_logits=False, debug_logits=False, async_mode=False, slot=0, run_steps=None, generator=None, seeds=None, guard=None, two_tile=False):
        """conds: one T3 cond dict (shared voice) or a list of B; text_tokens: list of B 1-D LongTensors that already
        carry SOT/EOT (mtl_tts.py:319-322).  Returns a list of B 1-D LongTensors (EOS included if it was sampled).
        temperature, top_p, min_p, repetition_penalty, cfg_weight: a scalar, or a sequence of B (one row of cbx_sampler_t.dev_params per utterance).
        generator: a torch.Generator on the engine's device for the sampling draws (None: the global RNG).
        seeds: None, or B ints in [0, 2^64) (an int: the same for every utterance) -- utterance b's draw of step i is column i of seeds[b]'s
        RNG_T3_UNIFORMS stream (ops.rng_fill), whatever its row and the batch around it; injected `uniforms` win; not together with a generator.
        `slot` selects an independent set of workspaces / KV cache / decode graph (pipelined serving keeps two alive).
        Chunked use (streaming synthesis): `async_mode=True, run_steps=k` samples only the first k tokens and returns a handle;
        `advance(handle, n)` enqueues n more decode steps and `peek(handle)` fetches the tokens sampled so far.
        guard: None, or a dict of check_guard's keys (missing ones take GUARD_DEFAULTS) -- the alignment guard: inside every token step, the attention mass
        the named heads put on the text columns (ops.guard_text_mass, after decode_attn_rope of their layers) drives a state machine per utterance
        (ops.guard_update, ahead of the sampler; include/cbx.h states it) that bans EOS until the text position has reached the last end_tokens text tokens and
        forces EOS once the mass stays on the last tokens (`tail`), goes back to earlier text (`repeat`) or the last token_run sampled tokens are one token
        (`run`).  Such a request takes the Python-sequenced step, replayed as a torch-captured graph kept beside the unguarded one.  Afterwards last_guard is the
        per-utterance report and last_guard_device the device tensors (mass history (B, max_steps, ld), trace, state, sums).  Not with ban_eos / ban_from, which
        ban the EOS the guard must be able to force; advance() refuses such a handle.  None: the call is launch for launch the one it always was.
        two_tile: a batch of 9 .. 16 utterances (17 .. 32 rows) decodes on the packed five-launch layer and the C step, two row tiles per launch (_packed_rows);
        every logit of every step is bit for bit the one the same utterance gets in a batch of at most 8.  False: the 9-launch step, as before."""
        dev, B = self.dev, len(text_tokens)
        assert B >= 1, "empty batch"
        guard = self.check_guard(guard)
        if guard is not None:
            if ban_eos or ban_from > 0:
                raise ValueError("guard together with ban_eos / ban_from: both ban the end-of-speech token the guard must be able to force")
            if max(int(t.numel()) for t in text_tokens) > 1024:
                raise ValueError(f"guard: {max(int(t.numel()) for t in text_tokens)} text tokens (at most 1024)")
        seeds = ops.request_seeds(seeds, B, generator)
        uniforms = self._uniform_rows(uniforms, B, max_new_tokens, f"max_new_tokens={max_new_tokens}")
        # {cfg_weight, temperature, min_p, top_p, rep_penalty, top_k, ban_token, ban_from} per utterance (cbx_sampler_t.dev_params); a wrong length raises here
        samp = sampler_rows(B, (("cfg_weight", cfg_weight), ("temperature", temperature), ("min_p", min_p), ("top_p", top_p),
                                ("repetition_penalty", repetition_penalty), ("top_k", 0.0), ("ban_token", float(STOP_SPEECH if ban_eos else -1)),
                                ("ban_from", float(ban_from))))
        if B > self.MAX_BATCH:  # rows = 2B feeds the decode GEMV (M <= 64): larger batches run as consecutive sub-batches
            assert not (async_mode or debug_logits or return_prefill_logits), "sub-batching is only defined for the plain token path"
            out, reports = [], []
            for lo in range(0, B, self.MAX_BATCH):
                hi = min(B, lo + self.MAX_BATCH)
                if lo and guard is not None:
                    reports += self.last_guard
                out += self.generate(conds if isinstance(conds, dict) else conds[lo:hi], text_tokens[lo:hi], max_new_tokens=max_new_tokens,
                                     temperature=_slice_param(temperature, lo, hi), top_p=_slice_param(top_p, lo, hi), min_p=_slice_param(min_p, lo, hi),
                                     repetition_penalty=_slice_param(repetition_penalty, lo, hi), cfg_weight=_slice_param(cfg_weight, lo, hi),
                                     uniforms=None if uniforms is None else uniforms[lo:hi], ban_eos=ban_eos,
                                     ban_from=ban_from, use_graph=use_graph, poll_every=poll_every, slot=slot, generator=generator,
                                     seeds=None if seeds is None else seeds[lo:hi], guard=guard, two_tile=two_tile)
            if guard is not None:
                self.last_guard = reports + self.last_guard
            return out
        rows = 2 * B
        prec = self.tune.get("prefill_prec") or 0
        # the conditioning prefix of every voice of the batch (VoicePrefixCache): cached -> pasted; a batch of ONE voice that misses runs the full prefill and keeps
        # that voice's K / V; a batch that MIXES voices computes the missing prefixes once per distinct voice (a prefix-only prefill), then every row prefills its
        # text positions only
        voices, voice_of = self._distinct_voices(conds, B)
        share = bool(self.share_prefix) and prec in (0, 1)
        ents = [self._voice_prefix(v) for v in voices] if share else [None] * len(voices)
        tl = [int(t.numel()) for t in text_tokens]
        s0 = [34 + n + 2 for n in tl]
        S = max(s0)
        max_ctx = (S + max_new_tokens + 63) // 64 * 64
        assert max_ctx <= self.max_pos, "context exceeds the RoPE table"
        st = self._get_state(B, max_ctx, max_new_tokens, slot)
        self._prepare_tune()
        if bool(st.get("two_tile")) != bool(two_tile):  # the captured step bakes its form in
            self._drop_c_step(st)
            st["graph"] = None
            st["two_tile"] = bool(two_tile)
        st["guard_on"] = None if guard is None else self._begin_guard(st, guard, tl, samp)  # (also: the first EOS ban into the request's sampler row)
        self._begin_request(st, samp, uniforms, max_new_tokens, generator, seeds)

        # ---- the missing prefixes of a mixed-voice batch: [conditioning] alone through the layers, once per distinct voice, into cache rows 0 .. n - 1
        missing = [j for j, e in enumerate(ents) if e is None]
        if share and missing and len(voices) > 1:
            xc = torch.stack([self.cond_embeds(voices[j]) for j in missing]).view(len(missing) * 34, self.D)
            self._prefill_rows(xc, 34, len(missing), st, torch.arange(34, dtype=torch.int32, device=dev).repeat(len(missing)),
                               torch.arange(len(missing), dtype=torch.int32, device=dev).repeat_interleave(34), prec)
            for i, j in enumerate(missing):
                ents[j] = self._keep_voice_prefix(voices[j], st, row=i, keep=len(voices))
            missing = []
        pre = None if missing else ents  # every voice cached: prefill the text positions only
        if pre is None:
            ce = torch.stack([self.cond_embeds(v) for v in voices])

        # ---- prefill embeddings (prepare_input_embeds + second BOS, t3.py:102-130,305-313): one launch for the batch (cbx_prefill_embed)
        P0 = 34 if pre is not None else 0  # prompt positions that are NOT computed in this call
        Sx = S - P0
        x, pos, crow, last = ops.prefill_embed(text_tokens, text_emb=self.text_emb, text_pos=self.text_pos, speech_emb=self.speech_emb, speech_pos=self.speech_pos,
                                               bos_id=START_SPEECH, n_bos=2, cfg=True, abs_pos=False, cond_lens=[34] * B,
                                               cond=None if pre is not None else ce, cond_slots=voice_of, pos0=P0)
        xf = x.view(rows * Sx, self.D)
        pws = dict(h=torch.empty(rows * Sx, self.D, device=dev), qkv=torch.empty(rows * Sx, 3 * self.D, device=dev),
                   att=torch.empty(rows * Sx, self.D, device=dev), g=torch.empty(rows * Sx, self.F, device=dev))
        # prefill_prec (tune / CBX_T3_TUNE="prefill_prec=6", opt-in, untimed): the prefill's plain projections (q/k/v, o, down) and its attention
        # on the bf16x6 split kernels (24 significand bits, fp32 range, accumulation error below the exact MFMA's own: DESIGN.md section 1)
        # instead of the exact fp32 MFMA; gate|up (SwiGLU epilogue) and every decode step stay exact
        if pre is not None:
            self._paste_voice_prefixes(pre, voice_of + voice_of, st)
            with ops.gemm_precision(prec):
                for i, lw in enumerate(self.layers):
                    self._layer_prefill_text(lw, xf, pws, Sx, S, rows, st["kc"][i], st["vc"][i], pos, crow)
        else:
            self._prefill_rows(xf, S, rows, st, pos, crow, prec, pws)
        if pre is None and share and len(voices) == 1:
            self._keep_voice_prefix(voices[0], st)
        hl = xf.index_select(0, last).contiguous()
        ops.layernorm(hl, self.norm, None, st["dws"]["h"], 1e-5, rms=True)
        ops.linear(st["dws"]["h"], self.head, st["logits"])
        prefill_logits = st["logits"].clone() if return_prefill_logits else None
        del x, xf, pws

        # ---- decode loop: positions / ctx_lens hold the state BEFORE the first sample (incremented by the sampler)
        s0t = torch.tensor(s0 + s0, dtype=torch.int32, device=dev)
        st["positions"].copy_(s0t - 1)
        st["ctx_lens"].copy_(s0t)
        step_logits = [st["logits"].clone()] if debug_logits else None
        self._sample(st)
        if debug_logits:
            use_graph = False
        c_loop = self._ready_step(st, use_graph)  # the library's token loop (one ctypes call), or the torch-captured graph replayed from here
        last = max_new_tokens if run_steps is None else max(1, min(max_new_tokens, int(run_steps)))
        # EOS is polled every `poll_every` steps unless the caller wants no synchronisation
        ran = self._replay(st, last - 1, 0 if (ban_eos or async_mode) else poll_every, c_loop, use_graph, step_logits, event_tag=(list(s0), rows))
        if async_mode:  # everything is enqueued on the current stream; no host synchronisation happened
            return dict(st=st, B=B, next_i=1 + ran, max_new_tokens=max_new_tokens, guard=st["guard_on"])
        out = self.collect(dict(st=st, B=B, guard=st["guard_on"]))
        if debug_logits:
            return out, torch.stack(step_logits)  # (steps, 2B, V)
        return (out, prefill_logits) if return_prefill_logits else out

    # ------------------------------------------------------------------ word timestamps: the alignment pass
    # (layer, head) pairs whose attention follows the text token being spoken: the set the reference project's later alignment analyser reads on the 30-layer
    # multilingual T3.  NOT measured on this project's kernels with trained weights for either checkpoint.
    ALIGN_HEADS = ((9, 2), (12, 15), (13, 11))
    last_alignment = None  # what the last align() call left on the device

    def check_align_heads(self, align_heads=None):
        """align_heads (None: ALIGN_HEADS) as a tuple of (layer, head) int pairs; a pair that does not exist in the loaded model is a ValueError."""
        heads = tuple((int(l), int(h)) for l, h in (self.ALIGN_HEADS if align_heads is None else align_heads))
        if not heads:
            raise ValueError("align_heads: no (layer, head) pair")
        for l, h in heads:
            if not (0 <= l < self.L and 0 <= h < self.H):
                raise ValueError(f"align_heads: (layer {l}, head {h}) does not exist in a model of {self.L} layers of {self.H} heads")
        by_layer = {}
        for l, h in heads:
            by_layer.setdefault(l, []).append(h)
        if any(len(v) > 16 for v in by_layer.values()):
            raise ValueError("align_heads: more than 16 heads of one layer")
        return heads

    # ------------------------------------------------------------------ the alignment guard (generate(guard=); include/cbx.h)
    # What is publicly described of the reference project's later analyser, with ALIGN_HEADS for the heads.  UNMEASURED here: nobody has run these numbers on
    # trained weights with these kernels, and with the wrong heads hold_eos can itself keep a request running to max_new_tokens.  Opt-in.
    GUARD_DEFAULTS = dict(heads=None, back=3, ahead=6, end_tokens=3, tail=5.0, repeat=5.0, repeat_skip=5, token_run=3, hold_eos=True, min_text=6)
    last_guard = None         # per-utterance reports of the last guarded generate() / collect()
    last_guard_device = None  # ... and the device tensors behind them

    def check_guard(self, guard):
        """generate's guard= argument -> None, or the complete dict: heads a tuple of (layer, head) pairs that exist (check_align_heads; None: ALIGN_HEADS), back,
        ahead, repeat_skip, token_run, min_text ints >= 0 (token_run not 1: that would hold at every step), end_tokens in 1 .. 3, tail and repeat floats >= 0 (inf: the rule is off), hold_eos a bool.  ValueError
        before anything is launched."""
        if guard is None:
            return None
        if not isinstance(guard, dict) or set(guard) - set(self.GUARD_DEFAULTS):
            raise ValueError(f"guard: expected None or a dict of {sorted(self.GUARD_DEFAULTS)}, got {guard!r}")
        g = dict(self.GUARD_DEFAULTS, **guard)
        g["heads"] = self.check_align_heads(g["heads"])
        for k in ("back", "ahead", "end_tokens", "repeat_skip", "token_run", "min_text"):
            if isinstance(g[k], bool) or not isinstance(g[k], (int, float)) or g[k] != g[k] or g[k] in (float("inf"), float("-inf")) or int(g[k]) != g[k] or g[k] < 0:
                raise ValueError(f"guard: {k} = {g[k]!r} (an int >= 0)")
            g[k] = int(g[k])
        if g["token_run"] == 1:
            raise ValueError("guard: token_run = 1 holds at every step (one token is always a run of one): 0 switches the rule off, 2 or more is a run")
        if not 1 <= g["end_tokens"] <= 3:
            raise ValueError(f"guard: end_tokens = {g['end_tokens']} outside 1 .. 3 (the device keeps three tail sums)")
        for k in ("tail", "repeat"):
            g[k] = float(g[k])
            if not g[k] >= 0.0:
                raise ValueError(f"guard: a negative threshold ({k} = {g[k]!r})")
        g["hold_eos"] = bool(g["hold_eos"])
        return g

    def _begin_guard(self, st, guard, tl, samp):
        """The guard's side of _begin_request: buffers (state, scratch, history, trace -- allocated with the state when a guarded request first needs them),
        thresholds and text lengths into device memory, state zeroed; samp (the host image of the sampler's rows) gets the ban frame 0 is sampled under.
        Returns st["guard_on"]: the settings plus the launch plan -- runs of consecutive heads of one layer, in list order, each with its first scratch slot."""
        B, dev, heads = st["B"], self.dev, guard["heads"]
        buf = st.get("guard")
        if buf is None or buf["p"].shape[0] < len(heads):
            # a text of this state has at most max_ctx - max_steps - 36 tokens (generate: max_ctx covers 34 + text + 2 BOS + max_new_tokens)
            ld = max(4, min(1024, (st["max_ctx"] - st["max_steps"] - 36 + 3) // 4 * 4))
            i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
            buf = st["guard"] = dict(p=torch.zeros(max(16, len(heads)), B, ld, device=dev), mass=torch.zeros(B, st["max_steps"], ld, device=dev), state=i32(B, 8),
                                     sums=torch.zeros(B, 4, device=dev), trace=i32(B, st["max_steps"]), thr=torch.zeros(B, ops.GUARD_NTHR, device=dev), t_len=i32(B))
            st.pop("guard_graphs", None)  # (a captured guarded step holds the old buffers: also those parked with another geometry)
            for parked in st.get("geom_cache", {}).values():
                parked.pop("guard_graphs", None)
        assert max(tl) <= buf["mass"].shape[2], "guard: the text does not fit the history of this state"
        row = [guard["back"], guard["ahead"], guard["end_tokens"], guard["tail"], guard["repeat"], guard["repeat_skip"], guard["token_run"],
               guard["min_text"] if guard["hold_eos"] else -1]
        buf["thr"].copy_(torch.tensor([row] * B, dtype=torch.float32))
        buf["t_len"].copy_(torch.tensor(tl, dtype=torch.int32))
        for k in ("state", "sums", "trace"):
            buf[k].zero_()
        for b in range(B):  # frame 0 passes no step: pos = 0, complete iff 0 >= m - end_tokens
            hold = guard["hold_eos"] and tl[b] >= guard["min_text"] and tl[b] > guard["end_tokens"]
            samp[b, 6] = float(STOP_SPEECH if hold else -1)
        runs = []
        for slot, (l, h) in enumerate(heads):
            if runs and runs[-1][0] == l:  # (check_align_heads admits at most 16 heads of one layer: a run fits one launch)
                runs[-1][2].append(h)
            else:
                runs.append((l, slot, [h]))
        by_layer = {}
        for l, slot, hs in runs:
            by_layer.setdefault(l, []).append((slot, hs))
        return dict(guard, by_layer=by_layer, n_sel=len(heads), text_tokens=list(tl))

    def _guard_mass(self, st, layer, qkv, ssq=None):
        """After decode_attn_rope of `layer`: the text mass of every conditional row's new query for the guard's heads of this layer, into their scratch slots."""
        buf = st["guard"]
        for slot, hs in st["guard_on"]["by_layer"].get(layer, ()):
            ops.guard_text_mass(qkv, st["positions"], self.cos, self.sin, st["kc"][layer], hs, st["done"], buf["t_len"], 34, 0.125, buf["p"][slot:], qkv_ssq=ssq,
                                rms_dim=self.D if ssq is not None else 0, rms_eps=1e-5, max_ctx=st["max_ctx"])

    def _guard_update(self, st):
        buf = st["guard"]
        ops.guard_update(buf["p"], buf["t_len"], st["step"], st["done"], buf["thr"], st["out_tokens"], buf["mass"], buf["state"], buf["sums"], buf["trace"],
                         st["logits"], self.V, STOP_SPEECH, st["samp_dev"], n_sel=st["guard_on"]["n_sel"])

    GUARD_REASONS = ("eos", "tail", "repeat", "run", "length")

    @ops.on_device
    def collect(self, handle):
        """DecodeRuntime.collect; a guarded handle also leaves last_guard -- per utterance dict(reason: "eos" (sampled), "tail" / "repeat" / "run" (forced by
        that rule) or "length" (max_new_tokens reached), tokens, fired_at, completed_at (None: never), position, text_tokens) -- from one small copy beside the
        token copy, and last_guard_device."""
        out = super().collect(handle)
        g = handle.get("guard")
        if g is not None:
            buf = handle["st"]["guard"]
            rep = []
            for b, (row, toks) in enumerate(zip(buf["state"].cpu().tolist(), out)):
                pos, complete, completed_at, fired, fired_at = row[:5]
                reason = self.GUARD_REASONS[fired] if fired else "eos" if len(toks) and int(toks[-1]) == STOP_SPEECH else "length"
                rep.append(dict(reason=reason, tokens=int(len(toks)), fired_at=fired_at if fired else None, completed_at=completed_at if complete else None,
                                position=pos, text_tokens=g["text_tokens"][b]))
            self.last_guard = rep
            self.last_guard_device = dict(buf, heads=g["heads"])
        return out

    @ops.on_device
    @torch.inference_mode()
    def align(self, text_tokens, tokens, align_heads=None, slot=0):
        """Which text token is being spoken at every speech token (frame) of a finished generate() call: right after generate() has collected the tokens, on the
        same state (`slot`), before anything else uses it.  text_tokens: the B 1-D id tensors generate() took; tokens: the B 1-D tensors it returned.
        A teacher-forced prefill of the conditional rows (cache rows 0 .. B - 1) over [text | BOS BOS | tok_0 .. tok_(n-2)] behind the voice prefix that is already
        in the cache, layer by layer through the launches of _layer_prefill_text, up to the highest layer align_heads names; at each named layer ONE
        ops.attn_text_mass launch adds that layer's heads -- frame i of utterance b is the query at position s0_b - 1 + i, the position whose logits sampled
        tok_i; the text columns are [34, 34 + tl_b); weight 1 / (number of heads) --, then ONE ops.align_path launch for the batch.  K / V of the text and speech
        positions of the conditional rows are overwritten: the request is finished.  Returns the host spans (list of B (tl_b, 2) int tensors: first frame, last
        frame + 1 per text token) and keeps last_alignment = dict(mass (B, N, M), spans (B, M, 2), frame_tok (B, N) on the device; n, m host lists; tokens: the
        sampled tokens the pass was forced with)."""
        heads = self.check_align_heads(align_heads)
        dev, B = self.dev, len(text_tokens)
        sts = [s for k, s in self._state.items() if k[3] == slot]
        if len(sts) != 1 or sts[0]["B"] != B or len(tokens) != B:
            raise ValueError(f"align: slot {slot} holds no finished request of {B} utterances")
        st = sts[0]
        tl, n = [int(t.numel()) for t in text_tokens], [int(t.numel()) for t in tokens]
        if min(tl) < 1 or min(n) < 1:
            raise ValueError(f"align: every utterance needs a text token and a sampled token (text {tl}, sampled {n})")
        if max(tl) > 1024:
            raise ValueError(f"align: {max(tl)} text tokens (at most 1024)")
        q0 = [t + 1 for t in tl]  # frame 0 is the second BOS: index tl + 1 of the block [text | BOS BOS | speech]
        Sx = max(a + m_ for a, m_ in zip(q0, n))
        S = 34 + Sx
        assert S <= st["max_ctx"], "align: the request does not fit its own KV cache"
        # ---- embeddings: what the prefill and the decode step use -- [text | BOS BOS] by cbx_prefill_embed, speech token i (the input behind tok_i) as
        # speech_emb[tok_i] + speech_pos[i + 1], the next_pos_ids of the sampler -- ragged ends are zeros, hidden from every real query by the causal mask
        xt, _, _, _ = ops.prefill_embed(text_tokens, text_emb=self.text_emb, text_pos=self.text_pos, speech_emb=self.speech_emb, speech_pos=self.speech_pos,
                                        bos_id=START_SPEECH, n_bos=2, cfg=False, abs_pos=False, cond_lens=[34] * B, cond=None, pos0=34)
        x = torch.zeros(B, Sx, self.D, device=dev)
        x[:, : xt.shape[1]] = xt
        for b in range(B):
            if n[b] > 1:
                ids = tokens[b][: n[b] - 1].to(dev, torch.int64)
                ops.embed(ids, self.speech_emb, x[b, q0[b] + 1: q0[b] + n[b]], table2=self.speech_pos,
                          ids2=torch.arange(1, n[b], dtype=torch.int32, device=dev))
        pos = (34 + torch.arange(Sx, dtype=torch.int32, device=dev)).repeat(B)
        crow = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(Sx)
        xf = x.view(B * Sx, self.D)
        pws = dict(h=torch.empty(B * Sx, self.D, device=dev), qkv=torch.empty(B * Sx, 3 * self.D, device=dev),
                   att=torch.empty(B * Sx, self.D, device=dev), g=torch.empty(B * Sx, self.F, device=dev))
        mass = torch.zeros(B, max(n), max(tl), device=dev)
        by_layer = {}
        for l, h in heads:
            by_layer.setdefault(l, []).append(h)
        ctx0 = [34 + a for a in q0]  # frame i sees the keys j <= s0 - 1 + i
        launched = [0]

        def text_mass(hs):
            def run(q4, kc):
                ops.attn_text_mass(q4[:, :, 0], kc[:B, :, :S].permute(0, 2, 1, 3), mass, hs, n, ctx0, [34] * B, tl, 0.125, weight=1.0 / len(heads),
                                   accumulate=launched[0] > 0, q0=q0)
                launched[0] += 1
            return run

        prec = self.tune.get("prefill_prec") or 0
        with ops.gemm_precision(prec if prec in (0, 1) else 0):  # (attention over the cache's K / V is exact fp32 only)
            for i in range(max(by_layer) + 1):
                self._layer_prefill_text(self.layers[i], xf, pws, Sx, S, B, st["kc"][i], st["vc"][i], pos, crow,
                                         after_rope=text_mass(by_layer[i]) if i in by_layer else None)
        spans, frame_tok = ops.align_path(mass, n, tl)
        self.last_alignment = dict(mass=mass, spans=spans, frame_tok=frame_tok, n=n, m=tl, tokens=[t.detach().cpu() for t in tokens])
        host = spans.cpu()
        return [host[b, : tl[b]] for b in range(B)]
