"""Kernel-level tests of cbx_t3_sample (csrc/sampler.hip) in every mode (-m gpu; the same bodies run on the SIMT emulator).

Method.  With cfg = 0 the logits row stride may be 0, so the B utterances of one launch share ONE logits row and differ only in
their uniform: a launch samples the inverse CDF of one filtered distribution at B known points.  With cfg = 1 the launch gets 2 B
rows (row b and B + b), built by expand-then-contiguous.  The points are u = 0 (must give the lowest surviving id), u = 1 - 2**-24
(the largest fp32 below 1: the top of the support) and a stratified grid in between.

Reference: oracle.ref_torch.process_logits (order 0) / process_logits_turbo (order 1) + sample_inverse_cdf, in fp32 as the oracle
is.  Next to it `_twin` evaluates the same pipeline in fp64; it is used ONLY to decide whether a (distribution, u) pair is
decidable: the kernel's __expf masses and fp32 block sums legitimately differ from the reference in the last bits, so
  (i)  every filter decision (min-p, top-k, top-p cut) must have a relative margin >= 1e-4 between the tested quantity and its
       threshold (fast-exp argument reduction: |x| * 2**-24 with |x| <= ~90, i.e. ~5e-6, plus a few ulps of the sums; 1e-4 leaves an
       order of magnitude).  Seeds whose distribution misses (i) are not used (the seed loop of `_cases`); deliberate ties are
       exempt for the tied ids and assert the HF rule (`scores < kth` removed: every tie is kept, a score one ulp below is cut) instead;
  (ii) u * total must be >= 1e-5 * total away from every edge of the surviving ids' cumulative distribution.
A random u misses (ii) with probability 2e-5 * (number of surviving ids), i.e. 16 % for an unfiltered 8194-id row: no choice of
seeds brings that under the 2 % cap.  So the grid is stratified-random and each point is then moved, inside [0, 1), to the nearest
spot that is 2e-5 away from the edges of a surviving id whose interval is wider than 4e-5 -- using the fp64 REFERENCE only.  Points
stay next to edges when they fell next to edges (so a CDF shifted by more than 2e-5 is seen), and ids narrower than 4e-5, which
(ii) can never decide, are not probed.  The cap itself (<= 2 % of the interior pairs of a cell set aside, no end probe ever) is
asserted in the test.  Every decidable pair must give the reference's token; no allowance.

The flat row (all logits equal) is the one distribution where the oracle's top-p is not a function of the distribution (its sort
order decides which half is removed); include/cbx.h's kernel keeps every id that ties with the arg-max, so there the expected
distribution is the uniform one.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

U_LAST = 1.0 - 2.0 ** -24
FILTER_MARGIN, EDGE_MARGIN, CAP = 1e-4, 1e-5, 0.02
POISON = 1e4
VS = (8194, 6563, 704, 1024, 1025, 2047)
REPS, TEMPS = (1.0, 1.2, 2.0), (1.0, 0.8, 0.3)
SHARES = {}  # cell name -> share of interior pairs set aside (printed; see the pull request)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _cell(order, V, shape="gauss", cfg=0, temperature=1.0, min_p=0.0, top_p=1.0, rep=1.0, top_k=0, ban=False, cfg_weight=0.5):
    return dict(order=order, V=V, shape=shape, cfg=cfg, temperature=temperature, min_p=min_p, top_p=top_p, rep=rep, top_k=top_k, ban=ban,
                cfg_weight=cfg_weight)


def _name(c):
    return "o{order} cfg{cfg} V{V} {shape} T{temperature} minp{min_p} topp{top_p} rep{rep} k{top_k} ban{ban}".format(**c)


def _matrix(order, small=False):
    cells = []
    if order == 0:
        combos = [(mp, tp) for mp in (0.0, 0.05, 0.3) for tp in (1.0, 0.9, 0.5, 0.05)]
        for i, (mp, tp) in enumerate(combos):
            cells.append(_cell(0, VS[i % 6], cfg=(i + 1) % 2, temperature=TEMPS[(i // 3) % 3], min_p=mp, top_p=tp, rep=REPS[i % 3], ban=i % 4 == 1))
        cells += [_cell(0, 8194, "peaked", cfg=1, temperature=0.8, min_p=0.05, top_p=0.9, rep=1.2), _cell(0, 1025, "peaked"),
                  _cell(0, 2047, "flat", min_p=0.05, top_p=0.5), _cell(0, 704, "flat", min_p=0.3, temperature=0.8),
                  _cell(0, 6563, "signed", top_p=0.9, rep=2.0), _cell(0, 8194, cfg=1, temperature=0.8, min_p=0.05, rep=1.2, ban=True)]
        if small:
            cells = [cells[i] for i in (2, 4, 5, 10, 13, 15)]  # V 704 / 1025 / 2047, cfg 0 / 1, all three filters, peaked, flat
    else:
        combos = [(k, tp) for k in (0, 1, 2, 50, 1000, "V-1", "V", "V+5") for tp in (1.0, 0.95, 0.5)]
        for i, (k, tp) in enumerate(combos):
            V = VS[i % 6]
            k = {"V-1": V - 1, "V": V, "V+5": V + 5}.get(k, k)
            cells.append(_cell(1, V, cfg=(i // 2) % 2, temperature=TEMPS[(i // 2) % 3], top_p=tp, rep=REPS[(i + 1) % 3], top_k=k, ban=i % 4 == 2))
        cells += [_cell(1, 8194, "peaked", top_k=50, top_p=0.95, temperature=0.8, rep=1.2), _cell(1, 1024, "flat", top_k=50, top_p=0.5),
                  _cell(1, 8194, "ties", top_k=50, rep=1.2), _cell(1, 704, "ties", top_k=2, temperature=0.8),
                  _cell(1, 6563, "signed", top_k=6563 * 3 // 4), _cell(1, 2047, "signed", top_k=50, top_p=0.95, rep=2.0, ban=True),
                  _cell(1, 6563, cfg=0, temperature=0.8, top_k=1000, top_p=0.95, rep=1.2, ban=True),
                  _cell(1, 704, "ulp", top_k=2), _cell(1, 8194, "ulp", top_k=50, top_p=0.95, rep=1.2)]
        if small:
            cells = [cells[i] for i in (2, 8, 10, 16, 22, 25, 27, 29, 31)]  # k 0 / 2 / 50 / V - 1 / V + 5, V 704 / 1025 / 2047, cfg 0 / 1, flat, ties, signed + bans
    return cells


def _row(cell, seed):
    """One logits row (V,) of the cell's shape, and the row of the unconditional branch."""
    V, shape = cell["V"], cell["shape"]
    g = _g(1000 * seed + V)
    if shape == "gauss":
        c = torch.randn(V, generator=g) * 2.0
    elif shape == "peaked":  # one id 30 above the rest
        c = torch.randn(V, generator=g) * 0.5
        c[(37 * seed + 11) % V] = c.max() + 30.0
    elif shape == "flat":
        c = torch.full((V,), 1.25)
    elif shape == "ties":  # four exact ties across the k-th value: ranks k - 2 .. k + 1
        c = torch.randn(V, generator=g) * 2.0
        idx = torch.argsort(c, descending=True)
        k = cell["top_k"]
        c[idx[max(0, k - 2): k + 2]] = c[idx[k - 1]].clone()
    elif shape == "ulp":  # ranks k - 2, k - 1 tie at the k-th value, ranks k, k + 1 sit ONE ulp below it: cut, although next to the threshold
        c = torch.randn(V, generator=g) * 2.0
        idx = torch.argsort(c, descending=True)
        k = cell["top_k"]
        v = c[idx[k - 1]].clone()
        c[idx[max(0, k - 2): k]] = v
        c[idx[k: k + 2]] = torch.nextafter(v, torch.tensor(-float("inf")))
    elif shape == "signed":  # both signs, magnitudes from 1e-3 to 10, +-0: the order-preserving integer key of top_k_filter
        c = torch.sign(torch.randn(V, generator=g)) * 10.0 ** (torch.rand(V, generator=g) * 4.0 - 3.0)
        c[5], c[6] = 0.0, -0.0
    else:
        raise ValueError(shape)
    if cell["cfg"] and shape in ("gauss", "peaked", "signed"):
        un = c - torch.randn(V, generator=g) * 0.5
    else:
        un = c.clone()  # (exact ties must survive the CFG combination)
    return c, un


def _twin(cell, c, un, seen_ids, ban_token, ban_from):
    """The pipeline in fp64: normalised probabilities (bans applied) and whether every filter decision has its margin."""
    V, ok = cell["V"], True
    c, un = c.double(), un.double()
    l = c + cell["cfg_weight"] * (c - un) if cell["cfg"] else c.clone()

    def penalty(l):
        s = l[seen_ids]
        l = l.clone()
        l[seen_ids] = torch.where(s < 0, s * cell["rep"], s / cell["rep"])
        return l

    def top_p(l, ok):
        if cell["top_p"] < 1.0:
            thr = 1.0 - cell["top_p"]
            sl, si = torch.sort(l)
            cp = sl.softmax(-1).cumsum(-1)
            ok = ok and float(((cp - thr).abs() / thr).min()) >= FILTER_MARGIN
            rm = cp <= thr
            rm[-1] = False
            l = l.masked_fill(torch.zeros_like(rm).scatter(0, si, rm), float("-inf"))
        return l, ok

    T = cell["temperature"]
    if cell["shape"] == "flat":
        l = torch.zeros(V, dtype=torch.float64)
    elif cell["order"] == 0:
        l = penalty(l) / T
        if cell["min_p"] > 0:
            pr = l.softmax(-1)
            thr = cell["min_p"] * pr.max()
            ok = ok and float((pr / thr - 1).abs().min()) >= FILTER_MARGIN
            l = l.masked_fill(pr < thr, float("-inf"))
        l, ok = top_p(l, ok)
    else:
        l = l / T
        k = cell["top_k"]
        if 0 < k < V:
            kth = torch.topk(l, k)[0][-1]
            below = l[l < kth]
            if cell["shape"] != "ulp":  # (deliberate: temperature 1, no CFG, so the fp32 comparison `score < kth` sees the stored values and is exact)
                ok = ok and float(kth - below.max()) >= FILTER_MARGIN * max(1.0, abs(float(kth)))
            l = l.masked_fill(l < kth, float("-inf"))
        l, ok = top_p(l, ok)
        l = penalty(l)
    pr = l.softmax(-1)
    if ban_token >= 0:
        pr[ban_token] = 0
    if ban_from > 0:
        pr[ban_from:] = 0
    tot = float(pr.sum())
    ok = ok and tot > 0 and float(pr[pr > 0].min()) / tot > 1e-30  # (no mass in fp32's underflow range: the cells are built that way)
    return (pr / tot if tot > 0 else pr), ok


def _oracle(cell, c, un, seen_ids, ban_token, ban_from):
    """The fp32 oracle's probabilities (bans applied as the engines' oracles apply them: softmax entries zeroed)."""
    from oracle import ref_torch as O
    V = cell["V"]
    if cell["shape"] == "flat":
        l = torch.zeros(V)
    elif cell["order"] == 0:
        l = O.process_logits(c, un, seen_ids, cell["cfg_weight"], cell["temperature"], cell["min_p"], cell["top_p"], cell["rep"])
    else:
        l0 = c + cell["cfg_weight"] * (c - un) if cell["cfg"] else c
        l = O.process_logits_turbo(l0, seen_ids, cell["temperature"], cell["top_k"], cell["top_p"], cell["rep"])
    pr = torch.softmax(l, -1)
    if ban_token >= 0:
        pr[ban_token] = 0
    if ban_from > 0:
        pr[ban_from:] = 0
    return pr


def _grid(pr64, n, seed):
    """n stratified points of [0, 1), each moved to the nearest spot 2 * EDGE_MARGIN inside a surviving id wider than 4 * EDGE_MARGIN."""
    u0 = (torch.arange(n, dtype=torch.float64) + torch.rand(n, generator=_g(seed), dtype=torch.float64)) / n
    surv = torch.nonzero(pr64 > 0).flatten()
    hi = pr64[surv].cumsum(0)
    lo = torch.cat([torch.zeros(1, dtype=torch.float64), hi[:-1]])
    wide = torch.nonzero(hi - lo > 4 * EDGE_MARGIN).flatten()
    assert wide.numel() > 0
    lo, hi = lo[wide] + 2 * EDGE_MARGIN, hi[wide] - 2 * EDGE_MARGIN
    j = torch.searchsorted(hi, u0).clamp(max=wide.numel() - 1)  # first wide interval that ends above u0 ...
    jm = (j - 1).clamp(min=0)                                    # ... or the one before it, whichever is nearer
    d = lambda jj: (lo[jj] - u0).clamp(min=0) + (u0 - hi[jj]).clamp(min=0)
    j = torch.where(d(jm) < d(j), jm, j)
    return torch.minimum(torch.maximum(u0, lo[j]), hi[j]).float()


def _decidable(pr64, u):
    surv = torch.nonzero(pr64 > 0).flatten()
    edges = torch.cat([torch.zeros(1, dtype=torch.float64), pr64[surv].cumsum(0)])
    t = u.double() * edges[-1]
    j = torch.searchsorted(edges, t).clamp(1, edges.numel() - 1)
    dist = torch.minimum((t - edges[j - 1]).abs(), (edges[j] - t).abs())
    tok = surv[(torch.searchsorted(edges, t, right=True) - 1).clamp(0, surv.numel() - 1)]
    return dist >= EDGE_MARGIN * edges[-1], tok


def _case(cell, seed, B):
    """Everything of one (cell, seed): rows, seen ids, bans, uniforms, the oracle's tokens, the decidable mask -- or None when the
    fp64 twin says that a filter decision of this distribution is closer than FILTER_MARGIN or that an end probe is not robust."""
    from oracle import ref_torch as O
    V = cell["V"]
    c, un = _row(cell, seed)
    comb = c + cell["cfg_weight"] * (c - un) if cell["cfg"] else c
    rank = torch.argsort(comb, descending=True)
    # ids with positive and with negative logits, among them ids that survive every cut and ids that never do
    seen_ids = torch.unique(torch.cat([rank[:3], rank[-3:], torch.randint(0, V, (10,), generator=_g(seed + 77))])) if cell["rep"] != 1.0 else torch.tensor([rank[0]])
    ban_token, ban_from = (int(rank[2]), V - V // 8) if cell["ban"] else (-1, 0)
    pr64, ok = _twin(cell, c, un, seen_ids, ban_token, ban_from)
    if not ok:
        return None
    surv = torch.nonzero(pr64 > 0).flatten()
    tails = pr64[surv].flip(0).cumsum(0)
    if bool(((tails > 2.0 ** -25) & (tails < 2.0 ** -23)).any()):  # u = 1 - 2**-24 next to an edge: not a robust end probe
        return None
    pr32 = _oracle(cell, c, un, seen_ids, ban_token, ban_from)
    assert torch.equal(torch.nonzero(pr32 > 0).flatten(), surv), f"{_name(cell)} seed {seed}: the fp32 oracle and its fp64 twin keep different ids"
    u = torch.cat([torch.zeros(1), _grid(pr64, B - 2, seed), torch.tensor([U_LAST])])
    want = torch.tensor([O.sample_inverse_cdf(pr32, float(x)) for x in u])
    dec, tok64 = _decidable(pr64, u)
    dec[0] = dec[-1] = True  # the end probes are never set aside
    assert int(want[0]) == int(surv[0]), "u = 0 gives the lowest surviving id"
    if float(pr64[surv[-1]]) >= 1e-6:
        assert int(want[-1]) == int(surv[-1]), "u = 1 - 2**-24 gives the highest surviving id"
    assert torch.equal(want[dec], tok64[dec]), f"{_name(cell)} seed {seed}: fp32 oracle and fp64 twin disagree on a decidable pair"
    return dict(cell=cell, seed=seed, c=c, un=un, seen_ids=seen_ids, ban_token=ban_token, ban_from=ban_from, u=u, want=want, dec=dec, surv=surv)


def _cases(cell, n, B):
    out = []
    for seed in range(1, 60):
        cs = _case(cell, seed, B)
        if cs is not None:
            out.append(cs)
        if len(out) == n:
            return out
    raise AssertionError(f"{_name(cell)}: fewer than {n} of 59 seeds give a distribution with decidable filters")


def _state(dev, B, rows, V, steps, seen_ids=None):
    d = dict(seen=torch.zeros(B, V, dtype=torch.uint8), step=torch.zeros(B, dtype=torch.int32), out_tokens=torch.full((B, steps), -7, dtype=torch.int64),
             done=torch.zeros(B, dtype=torch.int32), n_generated=torch.zeros(B, dtype=torch.int32), next_ids=torch.full((rows + 2,), -5, dtype=torch.int64),
             next_pos_ids=torch.full((rows + 2,), -5, dtype=torch.int32), positions=torch.full((rows + 2,), 9, dtype=torch.int32),
             ctx_lens=torch.full((rows + 2,), 10, dtype=torch.int32))
    if seen_ids is not None:
        d["seen"][:, seen_ids] = 1
    return {k: v.to(dev) for k, v in d.items()}


def _logits(dev, c, un, B, cfg):
    """(tensor, ld): pad columns hold POISON; cfg = 0: one shared row (ld = 0); cfg = 1: 2 B rows, ld > V."""
    V = c.numel()
    LD = V + 38
    pad = lambda x: torch.cat([x, torch.full((LD - V,), POISON)])
    if not cfg:
        return pad(c)[None].contiguous().to(dev), 0
    return torch.cat([pad(c)[None].expand(B, LD), pad(un)[None].expand(B, LD)]).contiguous().to(dev), LD


def _params(cell, cs):
    return dict(cfg_weight=cell["cfg_weight"], temperature=cell["temperature"], min_p=cell["min_p"], top_p=cell["top_p"], rep_penalty=cell["rep"],
                top_k=cell["top_k"], ban_token=cs["ban_token"], ban_from=cs["ban_from"])


_PKEYS = ("cfg_weight", "temperature", "min_p", "top_p", "rep_penalty", "top_k", "ban_token", "ban_from")  # the order of cbx_sampler_t.dev_params
_DECOY = dict(cfg_weight=3.0, temperature=7.0, min_p=0.9, top_p=0.01, rep_penalty=5.0, top_k=3, ban_token=1, ban_from=2)  # by-value fields when dev_params rules


def _launch(dev, cs, through_dev_params, u=None, params=None):
    """One launch of the case at the uniforms u (default: the case's own): the tokens (B,) on the host, after checking every state array."""
    from chatterbox_amd import ops
    cell, u = cs["cell"], cs["u"] if u is None else u
    V, B, cfg = cell["V"], u.numel(), cell["cfg"]
    rows = 2 * B if cfg else B
    logits, ld = _logits(dev, cs["c"], cs["un"], B, cfg)
    d = _state(dev, B, rows, V, 1, cs["seen_ids"])
    seen0 = d["seen"].cpu().clone()
    par = params if params is not None else [_params(cell, cs)] * B
    if through_dev_params:
        kw = dict(_DECOY, dev_params=torch.tensor([[float(p[k]) for k in _PKEYS] for p in par]).to(dev))
    else:
        assert all(p == par[0] for p in par)
        kw = dict(par[0])
    ops.t3_sample(logits=logits, ld=ld, V=V, B=B, cfg=cfg, order=cell["order"], eos_token=-1, uniforms=u.view(B, 1).contiguous().to(dev), max_steps=1, **kw, **d)
    tok = d["out_tokens"][:, 0].cpu()
    assert int(tok.min()) >= 0 and int(tok.max()) < V, f"{_name(cell)}: token outside the vocabulary (pad columns hold {POISON})"
    assert d["step"].tolist() == [1] * B and d["n_generated"].tolist() == [1] * B and d["done"].tolist() == [0] * B
    assert d["next_ids"].tolist() == tok.tolist() * (2 if cfg else 1) + [-5, -5], "next_ids: B rows (cfg = 0) / 2 B rows (cfg = 1), guard untouched"
    assert d["next_pos_ids"].tolist() == [1] * rows + [-5, -5] and d["positions"].tolist() == [10] * rows + [9, 9] and d["ctx_lens"].tolist() == [11] * rows + [10, 10]
    seen0[torch.arange(B), tok] = 1
    assert torch.equal(d["seen"].cpu(), seen0), "seen: exactly the sampled id is added"
    return tok


def _check(cs, tok, what):
    cell, dec, want = cs["cell"], cs["dec"], cs["want"]
    bad = torch.nonzero(dec & (tok != want)).flatten().tolist()
    assert not bad, (f"{_name(cell)} seed {cs['seed']} ({what}): {len(bad)} of {int(dec.sum())} decidable pairs differ, first: u = {float(cs['u'][bad[0]])!r} "
                     f"got {int(tok[bad[0]])} want {int(want[bad[0]])} (support {int(cs['surv'][0])} .. {int(cs['surv'][-1])}, {cs['surv'].numel()} ids)")


@pytest.mark.parametrize("order", [0, 1])
def test_sampler_matrix(dev, order, B=258, seeds=2, small=False):
    """Every cell of the matrix (module docstring): by value and through dev_params (identical tokens), against the oracle on every
    decidable pair and on both end probes; at most CAP of a cell's interior pairs set aside (asserted)."""
    for cell in _matrix(order, small):
        aside = total = 0
        for cs in _cases(cell, seeds, B):
            tok = _launch(dev, cs, False)
            _check(cs, tok, "by value")
            assert torch.equal(_launch(dev, cs, True), tok), f"{_name(cell)}: dev_params gives other tokens than the same settings by value"
            aside, total = aside + int((~cs["dec"]).sum()), total + B - 2
        SHARES[_name(cell)] = aside / total
        print(f"{_name(cell)}: {aside} / {total} interior pairs set aside")
        assert aside <= CAP * total, f"{_name(cell)}: {aside} of {total} pairs undecidable: over the cap of {CAP}"


@pytest.mark.parametrize("order", [0, 1])
def test_sampler_dev_params_per_utterance(dev, order, n=32, V=2047):
    """One launch whose utterances carry DIFFERENT settings (cbx_sampler_t.dev_params): each utterance samples what a by-value launch
    with its own settings samples at the same uniform.  Settings differ in every one of the eight parameters."""
    base = _cell(order, V, cfg=1, temperature=0.8, min_p=0.05, top_p=0.9, rep=1.2, top_k=50 if order else 0)
    cs = _cases(base, 1, n + 2)[0]
    alts = [dict(), dict(temperature=0.3, cfg_weight=0.0), dict(top_p=0.5, rep_penalty=2.0, top_k=2), dict(min_p=0.3, top_p=1.0, top_k=1000, ban_token=int(cs["surv"][0])),
            dict(top_k=7, ban_from=V - 300, cfg_weight=1.5), dict(top_k=6, temperature=1.0, ban_token=7, ban_from=0)]
    par = [dict(_params(base, cs), **alts[b % len(alts)]) for b in range(n + 2)]
    mixed = _launch(dev, cs, True, params=par)
    for a in range(len(alts)):
        own = _launch(dev, cs, False, params=[par[a]] * (n + 2))
        sel = torch.arange(a, n + 2, len(alts))
        assert torch.equal(mixed[sel], own[sel]), f"order {order}: utterances with settings {alts[a]} differ from their by-value launch"
    assert len({tuple(_launch(dev, cs, False, params=[par[a]] * (n + 2)).tolist()) for a in (0, 4, 5)}) == 3, "the settings do change the tokens"


@pytest.mark.parametrize("order,cfg", [(0, 1), (1, 0), (1, 1)])
def test_sampler_state_machine(dev, order, cfg, V=1025):
    """done[b] and step[b] == max_steps leave EVERY output array of that utterance untouched while its neighbours advance; a forced EOS sets done,
    writes the EOS id to next_ids of both CFG rows, and the next launch skips the utterance."""
    from chatterbox_amd import ops
    B, steps, eos = 5, 3, 1000
    rows = 2 * B if cfg else B
    c = torch.randn(V, generator=_g(3)) * 2.0
    lg = c[None].repeat(rows, 1)
    lg[2, eos] = lg[2].max() + 30.0  # utterance 2 is forced to EOS
    if cfg:
        lg[B + 2, eos] = lg[2, eos]
    d = _state(dev, B, rows, V, steps)
    d["done"][1] = 1            # finished earlier
    d["step"][3] = steps        # out of steps
    d["step"][4] = 1
    before = {k: v.cpu().clone() for k, v in d.items()}
    u = torch.rand(B, steps, generator=_g(4))
    kw = dict(logits=lg.to(dev), ld=V, V=V, B=B, cfg=cfg, order=order, cfg_weight=0.5, temperature=0.8, min_p=0.05, top_p=0.9, rep_penalty=1.2,
              top_k=50 if order else 0, ban_token=-1, ban_from=0, eos_token=eos, uniforms=u.to(dev), max_steps=steps)
    ops.t3_sample(**kw, **d)
    a = {k: v.cpu().clone() for k, v in d.items()}
    rws = lambda b: [b, B + b] if cfg else [b]
    for b in (1, 3):  # skipped utterances
        assert torch.equal(a["out_tokens"][b], before["out_tokens"][b]) and torch.equal(a["seen"][b], before["seen"][b])
        for k in ("step", "n_generated", "done"):
            assert int(a[k][b]) == int(before[k][b]), f"utterance {b}: {k} changed"
        for k in ("next_ids", "next_pos_ids", "positions", "ctx_lens"):
            assert a[k][rws(b)].tolist() == before[k][rws(b)].tolist(), f"utterance {b}: {k} changed"
    for b, s in ((0, 0), (2, 0), (4, 1)):  # advancing utterances: token at their own step index
        tok = int(a["out_tokens"][b, s])
        assert 0 <= tok < V and int(a["step"][b]) == s + 1 and int(a["n_generated"][b]) == s + 1 and int(a["seen"][b].sum()) == 1 and int(a["seen"][b, tok]) == 1
        assert a["out_tokens"][b].tolist() == [tok if i == s else -7 for i in range(steps)]
        assert a["next_ids"][rws(b)].tolist() == [tok] * len(rws(b)) and a["next_pos_ids"][rws(b)].tolist() == [s + 1] * len(rws(b))
        assert a["positions"][rws(b)].tolist() == [10] * len(rws(b)) and a["ctx_lens"][rws(b)].tolist() == [11] * len(rws(b))
    assert int(a["out_tokens"][2, 0]) == eos and a["done"].tolist() == [0, 1, 1, 0, 0]
    for k in ("next_ids", "next_pos_ids", "positions", "ctx_lens"):
        assert a[k][rows:].tolist() == before[k][rows:].tolist(), f"{k}: guard elements written"
        if not cfg:
            assert a[k][B:].tolist() == before[k][B:].tolist()
    ops.t3_sample(**kw, **d)  # second launch: utterance 2 is skipped now, 4 reaches max_steps - 1
    z = {k: v.cpu() for k, v in d.items()}
    for k in z:
        idx = rws(2) if k in ("next_ids", "next_pos_ids", "positions", "ctx_lens") else [2]
        assert torch.equal(z[k][idx], a[k][idx]), f"finished utterance: {k} changed in the next launch"
    assert z["step"].tolist() == [2, 0, 1, steps, 3] and z["positions"][rws(0)].tolist() == [11] * len(rws(0))


@pytest.mark.parametrize("cfg", [0, 1])
def test_sampler_no_mass_left_gives_the_best_allowed_raw_logit(dev, cfg, V=2047):
    """Order 1, top_k = 1, the arg-max banned by ban_from: total == 0.  include/cbx.h: the allowed id with the largest CFG-combined RAW logit
    (before temperature / penalty), lowest id on ties -- utterance 1 has an exact tie, utterance 2 a seen best id (the penalty must not matter)."""
    from chatterbox_amd import ops
    B, ban_from = 3, 1500
    rows = 2 * B if cfg else B
    c = torch.randn(B, V, generator=_g(9)) * 0.5
    c[:, 1800] = 30.0
    c[0, 1234], c[1, 700], c[1, 90], c[2, 1499] = 9.0, 8.0, 8.0, 7.0
    c[0, 1600] = 12.0  # banned too
    lg = torch.cat([c, c]) if cfg else c  # (uncond == cond: the combination is exact)
    d = _state(dev, B, rows, V, 1)
    d["seen"][2, 1499] = 1
    ops.t3_sample(logits=lg.to(dev), ld=V, V=V, B=B, cfg=cfg, order=1, cfg_weight=0.5, temperature=0.8, min_p=0.0, top_p=0.95, rep_penalty=1.2, top_k=1,
                  ban_token=1498, ban_from=ban_from, eos_token=-1, uniforms=torch.tensor([[0.0], [0.5], [U_LAST]]).to(dev), max_steps=1, **d)
    assert d["out_tokens"][:, 0].tolist() == [1234, 90, 1499]
    assert d["next_ids"].tolist() == [1234, 90, 1499] * (2 if cfg else 1) + [-5, -5]
