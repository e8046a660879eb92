"""CPU (-m "not gpu"): the alignment guard -- the NumPy state machine of guard_common.py on designed mass trajectories, each of which also runs step by step
through cbx_guard_update_f32 on the SIMT emulator and must agree exactly; both kernels on the emulator against the restatements, T3Engine.generate(guard=) on the emulator (a 2-layer synthetic model, B = 2, 5 steps: the device trace and reasons are the state machine
replayed over the device's own mass history and tokens, exactly), every refused argument, the C ABI, and the plumbing of guard= on the public classes over
recording engines (nothing is launched).  The recording engines build on those of test_seeded_rng_host.py (a read-only import)."""
import ctypes
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import guard_common as G  # noqa: E402
from test_seeded_rng_host import _FakeEngine, _tts  # noqa: E402  (read-only import: the recording engines)

CPU = torch.device("cpu")
HEADS = ((0, 3), (1, 5), (1, 9))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


# ----------------------------------------------------------------------------- the state machine on designed trajectories
def _walk(cols, m, thr, tokens=None, peak=0.6):
    """The state machine over peaked(m, cols) from step 1: list of update_ref's results (None once the row has fired), and the final state -- and the SAME
    trajectory through ops.guard_update on the emulator (guard_common.drive: history row, state, sums, trace, ban column and logits compared exactly at every
    step), so that what the assertions below say of the restatement is said of the kernel."""
    from chatterbox_amd import ops
    st = G.new_state(1)
    cols = list(cols)
    a = G.peaked(m, [0] + cols, peak)
    tokens = list(range(100, 100 + len(cols) + 2)) if tokens is None else tokens
    res = [G.update_ref(st, 0, a[i], m, i, thr, tokens) for i in range(1, len(cols) + 1)]
    fired = [i for i, r in enumerate(res, 1) if r is not None and r["reason"]]
    assert G.drive(ops, CPU, cols, m, thr, tokens, n_sel=1, peak=peak) == (fired[0] if fired else None)
    return res, st


def test_a_monotone_walk_never_fires_and_holds_eos_until_the_last_tokens(emu):
    m = 12
    res, st = _walk(range(1, m), m, G.thr_row())
    assert all(r["reason"] == 0 for r in res) and st["state"][0, 3] == 0
    for i, r in enumerate(res, 1):  # pos = i: EOS is banned exactly while pos < m - end_tokens
        assert (r["ban"] == G.EOS) == (i < m - 3), (i, r)
        assert r["trace"] == i | (i >= m - 3) << 16 | (i < m - 3) << 17
    assert st["state"][0, :3].tolist() == [m - 1, 1, m - 3]
    assert G.first_ban(m, G.thr_row()) == G.EOS and G.first_ban(5, G.thr_row()) == -1, "min_text = 6: a shorter text is never held"
    assert G.first_ban(m, G.thr_row(hold_eos=False)) == -1


def test_mass_that_stays_on_the_last_tokens_fires_tail_at_the_step_the_sum_crosses(emu):
    m = 10
    cols = list(range(1, m)) + [m - 1] * 12
    res, st = _walk(cols, m, G.thr_row(tail=3.0))
    fired = [i for i, r in enumerate(res, 1) if r is not None and r["reason"]]
    # the last column first holds the peak at step m - 1; its sum is 0.6 (k + 1) plus the small shares of the steps since completion: the crossing of 3.0
    a, s, want = G.peaked(m, [0] + cols), np.float32(0), None
    for i in range(m - 3, len(cols) + 1):
        s = np.float32(s + a[i, m - 1])
        if s >= 3.0:
            want = i
            break
    assert fired == [want] and res[want - 1]["reason"] == 1 and res[want - 1]["ban"] == -1 and st["state"][0, 3:5].tolist() == [1, want]
    assert all(r is None for r in res[want:]), "a row that has fired does nothing"


def test_mass_that_jumps_back_after_completion_fires_repeat(emu):
    m = 12
    cols = list(range(1, m - 2)) + [2] * 12   # complete at pos = 9 = m - 3, then the mass sits on an early token: outside the window, pos stays
    res, st = _walk(cols, m, G.thr_row(repeat=2.0))
    k = next(i for i, r in enumerate(res, 1) if r["reason"])
    assert res[k - 1]["reason"] == 2 and st["state"][0, 0] == m - 3, "the jump back is ignored by the position and counted by the repeat sum"
    assert k == (m - 3) + 4, "completed at step m - 3, whose add is the walk's own small share; then 0.6 per step: 2.0 is crossed by the 4th of those"
    assert _walk(cols, m, G.thr_row(repeat=2.0, repeat_skip=m))[1]["state"][0, 3] == 0, "repeat_skip >= m: no repeat column, the sum stays 0"


def test_a_token_run_fires_run_and_a_step_below_token_run_does_not(emu):
    m = 12
    toks = [7, 7, 7, 7, 9, 9, 9, 5]
    res, _ = _walk(range(1, 8), m, G.thr_row(), tokens=toks)
    assert [r["reason"] if r else None for r in res] == [0, 0, 3] + [None] * 4, "i = 1, 2 < token_run; i = 3 sees tokens 0 .. 2 equal"
    res, _ = _walk(range(1, 8), m, G.thr_row(token_run=0), tokens=toks)
    assert all(r["reason"] == 0 for r in res)
    res, _ = _walk(range(1, 8), m, G.thr_row(), tokens=[7, 7, 8, 9, 9, 9, 9, 5])
    assert [r["reason"] if r else None for r in res] == [0, 0, 0, 0, 0, 3, None]


def test_a_jump_outside_the_window_leaves_pos_and_a_tie_takes_the_lowest(emu):
    m = 20
    res, st = _walk([1, 2, 9, 3, 0, 7], m, G.thr_row())      # ahead = 6: 2 -> 9 is 7 ahead (ignored); back = 3: 3 -> 0 is allowed; 0 -> 7 is 7 ahead (ignored)
    assert [r["trace"] & 0xFFFF for r in res] == [1, 2, 2, 3, 0, 0]
    st = G.new_state(1)
    a = np.zeros(8, dtype=np.float32)
    a[[2, 5]] = 0.4
    assert G.update_ref(st, 0, a, 8, 1, G.thr_row(), [1, 2])["trace"] & 0xFFFF == 2, "the lowest t with the largest a[t]"
    from chatterbox_amd import ops
    assert G.drive(ops, CPU, [1, 2, 3], 12, G.thr_row(), list(range(100, 110)), tie=True) is None, "... on the kernel: every step has two equal largest columns"


@pytest.mark.parametrize("m", [1, 2, 3, 5, 6])
def test_short_texts(emu, m):
    thr = G.thr_row(tail=1.0, repeat=1.0, min_text=0)
    assert G.first_ban(m, thr) == (G.EOS if m > 3 else -1), "m <= end_tokens is complete at once: nothing to hold"
    res, st = _walk([min(i, m - 1) for i in range(1, 9)], m, thr, peak=0.5)
    k = next(i for i, r in enumerate(res, 1) if r["reason"])
    assert res[k - 1]["reason"] == 1, "the tail crosses first"
    assert st["state"][0, 2] == (1 if m <= 4 else m - 3) and (st["sums"][0, 3] == 0.0) == (m <= 5), "m <= repeat_skip = 5: no repeat column, the sum stays 0"
    assert (st["sums"][0, min(3, m):3] == 0).all(), "min(end_tokens, m) tail sums are used"


# ----------------------------------------------------------------------------- the kernels on the emulator
@pytest.mark.parametrize("t_len,ctx,nparts", [(1, 35, 0), (2, 36, 2), (5, 255, 4), (63, 256, 0), (64, 257, 2), (65, 34 + 65, 4), (7, [41, 300, 64], 2)],
                         ids=["t1", "t2", "t5", "t63", "t64", "t65", "ragged_positions"])
def test_guard_text_mass_on_the_emulator(emu, t_len, ctx, nparts):
    from chatterbox_amd import ops
    B, heads = 3, [0, 3, 3]
    c = G.mass_case(B, 4, ctx, [t_len, 1, t_len], nparts, 7 * t_len + nparts)
    done = [0, 0, 1]
    p = G.run_mass(ops, CPU, c, heads, done=done, slots=4)
    print(f"t_len {t_len}, context {ctx}, {nparts} parts: worst err / (1 + |ref|) = {G.check_mass(p, c, heads, done=done):.3g}")
    clean = G.mass_case(B, 4, ctx, [t_len, 1, t_len], nparts, 7 * t_len + nparts, poison=False)
    assert np.array_equal(p, G.run_mass(ops, CPU, clean, heads, done=done, slots=4)), "NaN nobody reads changed a result"
    assert np.array_equal(p, G.run_mass(ops, CPU, c, heads, done=done, slots=4)), "two runs are bit-identical"


def test_guard_text_mass_wide_scores_and_no_rope_on_the_emulator(emu):
    from chatterbox_amd import ops
    c = G.mass_case(1, 2, 300, 65, 0, 9, spread=27.0, rope=False)   # scores of about +-80
    G.check_mass(G.run_mass(ops, CPU, c, [1]), c, [1])
    c = G.mass_case(2, 2, 40, [6, 7], 2, 10)                        # a row whose text is not yet visible writes nothing
    c["t_len"][1] = 8                                                # 34 + 8 > 41
    p = G.run_mass(ops, CPU, c, [0])
    assert (p[0, 1] == -7.0).all() and (p[0, 0, :6] != -7.0).all()


@pytest.mark.parametrize("m", [1, 3, 6, 64, 65])
def test_guard_update_on_the_emulator(emu, m):
    from chatterbox_amd import ops
    toks = list(range(100, 140))
    walk = list(range(min(6, m - 1), m - 1, 6)) + [m - 1]   # steps of `ahead` to the last token
    assert G.drive(ops, CPU, walk + [m - 1] * 6, m, G.thr_row(tail=2.0, min_text=0), toks) is not None, "tail"
    if m > 8:
        assert G.drive(ops, CPU, list(range(6, m, 6)) + [m - 1, 2, 2, 2, 2, 2], m, G.thr_row(repeat=1.5), toks, n_sel=3) is not None, "repeat"
        assert G.drive(ops, CPU, [1, 2, 3, 4, 5], m, G.thr_row(), [7, 7, 8, 8, 8, 8, 1]) == 5, "run; steps 1, 2 < token_run"
        assert G.drive(ops, CPU, [1, 2, 20, 3, 0, 40], m, G.thr_row(), toks, n_sel=1) is None, "jumps outside the window"


def test_guard_update_rows_that_do_nothing_on_the_emulator(emu):
    from chatterbox_amd import ops
    st = G.new_state(3)
    st["state"][2, 3] = 2     # row 2 has fired before
    a = G.peaked(6, [1, 2, 3])
    d = G.run_update(ops, CPU, a, [6, 6, 6], [1, 1, 1], [G.thr_row()] * 3, st, [[5, 6]] * 3, done=[1, 0, 0])
    assert (d["trace"][[0, 2]] == -9).all() and d["trace"][1, 1] == (2 | 1 << 17) and (d["dp"][[0, 2]] == 0.25).all() and d["dp"][1, 6] == G.EOS
    assert (d["mass"][[0, 2]] == d["sentinel"]).all() and st["state"][0].tolist() == [0] * 8 and st["state"][2].tolist() == [0, 0, 0, 2, 0, 0, 0, 0]


# ----------------------------------------------------------------------------- the engine on the emulator
def test_guarded_generate_on_the_emulator_is_the_state_machine_over_its_own_history(emu):
    from chatterbox_amd import synth
    from chatterbox_amd.t3 import T3Engine
    eng = T3Engine(synth.t3_state_dict(2, 0), CPU)
    texts = [synth.text_tokens(n, seed=s) for n, s in ((3, 1), (7, 2))]
    conds = [synth.t3_cond(seed=s, prompt_len=20) for s in (2, 3)]
    steps = 5
    guard = dict(heads=HEADS, end_tokens=2, tail=0.6, repeat=0.5, repeat_skip=2, token_run=2, min_text=2)
    toks = eng.generate(conds, texts, max_new_tokens=steps, uniforms=synth.rand((2, steps), seed=11), use_graph=False, guard=guard, temperature=0.8, cfg_weight=0.5,
                        repetition_penalty=1.2, min_p=0.05, top_p=1.0)
    st = next(iter(eng._state.values()))
    assert "cstep" not in st and st["guard_on"]["heads"] == HEADS and [s for s, _ in sum(st["guard_on"]["by_layer"].values(), [])] == [0, 1], \
        "the Python-sequenced step; two launches: head 3 of layer 0, heads 5 and 9 of layer 1 in one"
    d, rep = eng.last_guard_device, eng.last_guard
    thr = G.thr_row(**{k: v for k, v in guard.items() if k != "heads"})
    assert np.array_equal(d["thr"].numpy(), np.asarray([thr] * 2, dtype=np.float32))
    for b in range(2):
        m, tk = int(texts[b].numel()), toks[b].tolist()
        mass = d["mass"][b].numpy()
        assert 0.0 < mass[1: len(tk), :m].sum(1).min() and mass[1: len(tk), :m].sum(1).max() <= 1.0 + 1e-5, "a step's text mass is a share of its attention"
        trace, state, sums = G.replay(mass, tk, m, thr, steps)
        assert d["trace"][b].tolist() == trace and d["state"][b].tolist() == state.tolist() and np.array_equal(d["sums"][b].numpy(), sums), (b, trace, d["trace"][b])
        fired = int(state[3])
        assert rep[b]["reason"] == (("eos", "tail", "repeat", "run")[fired] if fired or tk[-1] == G.EOS else "length")
        assert rep[b]["tokens"] == len(tk) and rep[b]["text_tokens"] == m and rep[b]["position"] == int(state[0])
        if fired:
            assert tk[-1] == G.EOS and len(tk) == int(state[4]) + 1 == rep[b]["fired_at"] + 1, "the sampler itself wrote the forced end token"
    print("reports:", rep)
    # repeat = 0 holds at completion: a row that completed at step c of the run above is forced there, and the sampler writes the end token at index c
    done_at = [r["completed_at"] for r in rep]
    assert any(c is not None and c < steps for c in done_at), "the texts (5 and 9 tokens, end_tokens = 2) were chosen to complete within 5 steps"
    short = eng.generate(conds, texts, max_new_tokens=steps, uniforms=synth.rand((2, steps), seed=11), use_graph=False, guard=dict(guard, repeat=0.0), temperature=0.8,
                         cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0)
    thr0 = G.thr_row(**{k: v for k, v in dict(guard, repeat=0.0).items() if k != "heads"})
    for b, c in enumerate(done_at):
        if rep[b]["reason"] == "length" and c is not None and c < steps:
            assert short[b].tolist() == toks[b].tolist()[:c] + [G.EOS] and eng.last_guard[b]["reason"] == "repeat" and eng.last_guard[b]["fired_at"] == c
        assert eng.last_guard_device["trace"][b].tolist() == G.replay(eng.last_guard_device["mass"][b].numpy(), short[b].tolist(), int(texts[b].numel()), thr0, steps)[0]
    with pytest.raises(ValueError, match="advance"):
        eng.advance(dict(st=st, B=2, next_i=steps, max_new_tokens=steps, guard=st["guard_on"]), 1)


# ----------------------------------------------------------------------------- arguments and ABI
def _bare_engine(L=2):
    from chatterbox_amd.t3 import T3Engine
    eng = T3Engine.__new__(T3Engine)
    eng.L = L
    return eng


def test_what_generate_refuses_before_any_launch():
    from chatterbox_amd.t3 import T3Engine
    eng = _bare_engine()
    ok = dict(heads=HEADS)
    for bad, match in ((dict(ok, heads=((2, 0),)), "layer 2"), (dict(ok, heads=((0, 16),)), "head 16"), (dict(ok, end_tokens=0), "end_tokens"), (dict(ok, end_tokens=4), "end_tokens"),
                       (dict(ok, tail=-1.0), "negative"), (dict(ok, repeat=-0.5), "negative"), (dict(ok, tail=float("nan")), "negative"), (dict(ok, back=-1), "back"),
                       (dict(ok, token_run=1.5), "token_run"), (dict(ok, token_run=1), "token_run = 1"), (dict(ok, hold=True), "guard"), ("on", "guard"), (dict(), "layer 9")):
        with pytest.raises(ValueError, match=match):
            eng.check_guard(bad)
    g = eng.check_guard(ok)
    assert g == dict(T3Engine.GUARD_DEFAULTS, heads=HEADS) and eng.check_guard(None) is None
    assert T3Engine.GUARD_DEFAULTS == dict(heads=None, back=3, ahead=6, end_tokens=3, tail=5.0, repeat=5.0, repeat_skip=5, token_run=3, hold_eos=True, min_text=6)
    assert eng.check_guard(dict(ok, tail=float("inf"), repeat=0))["tail"] == float("inf")
    eng.dev = CPU
    texts = [torch.zeros(3, dtype=torch.long)]
    for kw in (dict(ban_eos=True), dict(ban_from=5)):
        with pytest.raises(ValueError, match="ban_eos / ban_from"):
            eng.generate({}, texts, guard=ok, **kw)
    with pytest.raises(ValueError, match="1024"):
        eng.generate({}, [torch.zeros(1025, dtype=torch.long)], guard=ok)
    with pytest.raises(ValueError, match="advance"):
        eng.advance(dict(st={}, guard=g, max_new_tokens=4, next_i=1), 1)


def test_guard_off_is_the_parents_step():
    """No guard: the state takes the C step / the library's token loop as before and no guard launch is reachable; a guarded state does not."""
    from chatterbox_amd.t3 import T3Engine
    eng = _bare_engine()
    eng.c_step, eng.decode_mode, eng.tune = True, "v2", dict(T3Engine._TUNE)
    st = dict(rows=4)
    assert eng._use_c_step(st) and eng._graph_slot(st) == (st, "graph")
    st["guard_on"] = None
    assert eng._use_c_step(st) and eng._graph_slot(st) == (st, "graph")
    st["guard_on"] = dict(heads=HEADS)
    d, k = eng._graph_slot(st)
    assert not eng._use_c_step(st) and d is st["guard_graphs"] and k == HEADS, "one captured graph per set of heads, beside the unguarded one"
    # whoever takes a state next starts unguarded (measure_decode / probe_decode never set the flag themselves)
    eng._state = {(2, 64, 8, 7): st}
    assert eng._get_state(2, 64, 8, 7) is st and st["guard_on"] is None and eng._use_c_step(st)


def test_entry_points_are_declared_exported_bound_and_documented():
    from chatterbox_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    for e in ("cbx_guard_text_mass_f32", "cbx_guard_update_f32"):
        assert re.search(rf"^int {e}\(", hdr, re.M) and hasattr(lib, e) and e in _lib._SIGS, e
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.lib.cbx_abi_version() == 16 and _lib.ABI_VERSION == 16, "new functions only: no version step"
    block = hdr[hdr.index("---- alignment guard"): hdr.index("int cbx_guard_update_f32(")]
    for phrase in ("over ALL visible keys j <= positions[b]", "in part order", "A key beyond positions[b] is never loaded", "done[b] != 0 writes nothing", "max_ctx <= 4608",
                   "t_cap <= 1024", "-22 before any launch, nothing written", "the lowest t with the largest a[t]", "a jump outside the window is ignored",
                   "pos | complete << 16 | ban << 17 | reason << 18", "32768", "Columns v >= V of a padded row are not touched", "the first call sees i = 1 and pos = 0"):
        assert phrase in block, phrase
    src = open(os.path.join(ROOT, "chatterbox_amd", "csrc", "t3_guard.hip")).read()
    assert "asm" not in src.replace("inline assembly", "") and "atomic" not in src.replace("no\n// atomics", "").replace("no atomics", ""), "plain C++, no atomics"
    assert callable(ops.guard_text_mass) and callable(ops.guard_update)


def test_refused_descriptors_return_a_status_and_write_nothing():
    """on host buffers: a launch of the product library on them would fault, a refusal never gets that far"""
    from chatterbox_amd import _lib
    lib = _lib.lib
    f, i = (ctypes.c_float * 4096)(*[7.0] * 4096), (ctypes.c_int * 64)()
    fa, ia = ctypes.addressof(f), ctypes.addressof(i)

    def mass_call(heads=(0,), n_sel=1, B=1, nparts=0, ssq=None, rms_dim=0, ld_qkv=384, kc=fa, k_sh=64 * 8, max_ctx=8, t_cap=4, p_sb=4, p=fa, sin=fa):
        return lib.cbx_guard_text_mass_f32(fa, ld_qkv, nparts, 0, ssq, rms_dim, 1e-5, ia, fa, sin, kc, 1024, k_sh, max_ctx, G.W.c_ints(list(heads)), n_sel, 2, B, ia, ia, 34,
                                           t_cap, 0.125, p, 64, p_sb, None)
    for bad in (dict(p=None), dict(sin=None), dict(heads=(2,)), dict(heads=(-1,)), dict(n_sel=0), dict(n_sel=17), dict(B=0), dict(B=65), dict(nparts=3), dict(nparts=2),
                dict(nparts=2, ssq=fa), dict(nparts=2, ssq=fa, rms_dim=8, B=17), dict(ld_qkv=127), dict(kc=fa + 4), dict(k_sh=66), dict(max_ctx=0), dict(max_ctx=4609),
                dict(max_ctx=9), dict(t_cap=0), dict(t_cap=1025), dict(p_sb=3)):
        assert mass_call(**bad) == -22 and b"guard_text_mass" in lib.cbx_last_error(), bad

    def update_call(n_sel=1, B=1, max_steps=4, V=8, eos=2, ld=8, m_si=4, m_sb=16, state=ia):
        return lib.cbx_guard_update_f32(fa, 64, 4, n_sel, ia, ia, ia, fa, ia, max_steps, fa, m_sb, m_si, state, fa, ia, fa, ld, V, B, eos, fa, None)
    for bad in (dict(state=None), dict(n_sel=0), dict(B=0), dict(B=65), dict(max_steps=0), dict(V=0), dict(eos=8), dict(eos=-1), dict(ld=7), dict(m_si=0), dict(B=2, m_sb=15)):
        assert update_call(**bad) == -22 and b"guard_update" in lib.cbx_last_error(), bad
    assert all(v == 7.0 for v in f) and all(v == 0 for v in i), "a refused call writes nothing"


# ----------------------------------------------------------------------------- plumbing over recording engines
class _GuardEngine(_FakeEngine):
    """records like _FakeEngine; a guarded call / job leaves last_guard: request of n text tokens ends by "tail" when n is odd, else by "eos" """
    last_guard = None

    def _report(self, text_tokens):
        return [dict(reason="tail" if t.numel() % 2 else "eos", tokens=int(t.numel()), fired_at=None, completed_at=None, position=0, text_tokens=int(t.numel())) for t in text_tokens]

    def synthesize(self, text_tokens, t3_conds, gen_ref, **kw):
        self.last_guard = self._report(text_tokens) if kw.get("guard") is not None else None
        if kw.get("join") is not None:
            self.calls.append(("synthesize", dict(text_tokens=text_tokens, **kw)))
            n = len(text_tokens)
            return dict(wav=torch.zeros(4 * n), total=4 * n, offsets=[4 * r for r in range(n)], edges=[(0, 4)] * n, truncated=[False] * n, n=[4] * n), None
        return super().synthesize(text_tokens, t3_conds, gen_ref, **kw)

    def synthesize_pipelined(self, jobs, **kw):
        self.calls.append(("pipelined", dict(jobs=jobs, **kw)))
        for job in jobs:
            self.last_guard = self._report(job["text_tokens"]) if job.get("guard") is not None else None
            if "join" in job:
                n = len(job["text_tokens"])
                yield dict(wav=torch.zeros(4 * n), total=4 * n, offsets=[4 * r for r in range(n)], edges=[(0, 4)] * n, truncated=[False] * n, n=[4] * n), None, 0.0
            else:
                yield [torch.full((3,), float(t.numel())) for t in job["text_tokens"]], None, 0.0


def _model(cls_name="ChatterboxTTS"):
    from chatterbox_amd import api
    return _tts(getattr(api, cls_name), _GuardEngine())


@pytest.mark.parametrize("cls_name", ["ChatterboxTTS", "ChatterboxMultilingualTTS"])
def test_no_guard_records_the_calls_of_the_parent(cls_name):
    lang = ("en",) if cls_name == "ChatterboxMultilingualTTS" else ()
    a, b = _model(cls_name), _model(cls_name)
    a.generate("Hi there.", *lang, seed=3)
    b.generate("Hi there.", *lang, seed=3, guard=None)
    a.generate_batch(["Hi there.", "Yes."], *(["en"] if lang else []), seeds=[1, 2])
    b.generate_batch(["Hi there.", "Yes."], *(["en"] if lang else []), seeds=[1, 2], guard=False)
    a.generate_long("Hi there. Yes.", *lang, seed=4)
    b.generate_long("Hi there. Yes.", *lang, seed=4, guard=None)
    assert len(a.engine.calls) == len(b.engine.calls) == 3 and b.last_guard is None
    for (ka, kwa), (kb, kwb) in zip(a.engine.calls, b.engine.calls):
        assert ka == kb and sorted(kwa) == sorted(kwb) and "guard" not in str(kwb) and str(kwa) == str(kwb)


@pytest.mark.parametrize("cls_name", ["ChatterboxTTS", "ChatterboxMultilingualTTS"])
def test_guard_travels_to_the_engine_and_the_reports_come_back_in_the_callers_order(cls_name):
    from chatterbox_amd.t3 import T3Engine
    lang = ("en",) if cls_name == "ChatterboxMultilingualTTS" else ()
    m = _model(cls_name)
    m.align_heads = HEADS
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m.generate("Hi.", *lang, guard=True)          # 3 characters + start / end (+ the language token): the recording engine says why by the count's parity
    kw = m.engine.calls[-1][1]
    assert kw["guard"] == dict(T3Engine.GUARD_DEFAULTS, heads=HEADS), "True: the defaults, with the model's align_heads"
    n = int(kw["text_tokens"][0].numel())
    assert len(m.last_guard) == 1 and m.last_guard[0]["reason"] == ("tail" if n % 2 else "eos")
    assert bool(w) == bool(n % 2) and all(issubclass(x.category, UserWarning) and "'tail'" in str(x.message) for x in w)
    m.generate("Hi.", *lang, guard=dict(tail=2.0, heads=((0, 1),)))
    assert m.engine.calls[-1][1]["guard"] == dict(T3Engine.GUARD_DEFAULTS, heads=((0, 1),), tail=2.0), "a dict overrides single keys"
    for bad in (dict(tails=1.0), "yes", 3):
        with pytest.raises(ValueError, match="guard"):
            m.generate("Hi.", *lang, guard=bad)
    # a batch: sub-batches in order of text length through the throughput schedule; the reports follow their requests
    m.max_batch = 2
    texts = ["Hi yo.", "A.", "Hi yo, a.", "Abcd."]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m.generate_batch(texts, *(["en"] if lang else []), seeds=[1, 2, 3, 4], guard=True)
    kind, kw = m.engine.calls[-1]
    assert kind == "pipelined" and all(job["guard"] == dict(T3Engine.GUARD_DEFAULTS, heads=HEADS) for job in kw["jobs"]), "one setting for the call, both slots"
    extra = [r["text_tokens"] - len(t) for r, t in zip(m.last_guard, texts)]
    assert len(set(extra)) == 1, "request i's report is the one of ITS text"
    odd = [i for i, r in enumerate(m.last_guard) if r["reason"] != "eos"]
    assert (len(w) == 1 and all(f"{i} by 'tail'" in str(w[0].message) for i in odd)) if odd else not w
    # long form: every chunk guarded, its report in its segment
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        wav, segs = m.generate_long("Hello there. Numbers one two three. Hi.", *lang, max_chars=20, seed=5, return_segments=True, guard=True)
        assert len(segs) >= 2 and all(s["guard"]["reason"] in ("eos", "tail") for s in segs) and m.last_guard == [s["guard"] for s in segs]
        pieces = list(m.generate_long_stream("Hello there. Numbers one two three. Hi.", *lang, max_chars=20, seed=5, return_segments=True, guard=True))
        assert [s["guard"] for _, ss in pieces for s in ss] == m.last_guard and len(m.last_guard) == len(segs)
    _, plain = m.generate_long("Hello there. Numbers one two three. Hi.", *lang, max_chars=20, seed=5, return_segments=True)
    assert all("guard" not in s for s in plain)


def test_what_does_not_take_the_argument_and_what_the_engine_refuses():
    import inspect
    from chatterbox_amd import api, engine as E
    for cls_name, method in (("ChatterboxTTS", "generate_stream"), ("ChatterboxMultilingualTTS", "generate_stream"), ("ChatterboxTurboTTS", "generate"),
                             ("ChatterboxTurboTTS", "generate_batch"), ("ChatterboxTurboTTS", "generate_long"), ("ChatterboxVC", "generate")):
        assert "guard" not in inspect.signature(getattr(getattr(api, cls_name), method)).parameters, (cls_name, method)
    with pytest.raises(TypeError, match="guard"):
        _model().generate_stream("Hi.", guard=True)
    for method in ("generate", "generate_batch", "generate_long", "generate_long_stream"):
        for cls_name in ("ChatterboxTTS", "ChatterboxMultilingualTTS"):
            assert inspect.signature(getattr(getattr(api, cls_name), method)).parameters["guard"].default is None
    assert "UNMEASURED" in api.ChatterboxTTS.generate.__doc__.split("guard (None;")[1], "the defaults are stated as unmeasured where the argument is described"
    job = dict(text_tokens=[torch.zeros(3, dtype=torch.long)], t3_conds=None, gen_ref=None)
    assert "guard" not in E._checked_job(dict(job, guard=None)) and E._checked_job(dict(job, guard=dict(tail=1.0)))["guard"] == dict(tail=1.0)
    assert inspect.signature(E.ChatterboxEngine.synthesize).parameters["guard"].default is None
    eng = E.ChatterboxEngine.__new__(E.ChatterboxEngine)
    eng.dev, eng.t3 = CPU, _bare_engine()
    for kw in (dict(ban_eos=True), dict(ban_from=3)):
        with pytest.raises(ValueError, match="ban_eos / ban_from"):
            eng.synthesize(job["text_tokens"], None, None, guard=dict(heads=HEADS), **kw)
    with pytest.raises(ValueError, match="end_tokens"):
        eng.synthesize(job["text_tokens"], None, None, guard=dict(heads=HEADS, end_tokens=5))
