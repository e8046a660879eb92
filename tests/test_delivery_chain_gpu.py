"""GPU (-m gpu): the chain behind the vocoder on a bare S3GenEngine (synthetic weights) with every delivery option on -- seeds, speed, pitch, loudness, pauses and a
mulaw 8 kHz format over three rows of 12, 5 and 9 tokens, two CFM steps.  vocode on the default stream with sync=True and vocode with hift_stream= the engine's
vocoder stream and sync=False (finished through ops.cut_pauses after a synchronise) make the same launches on the fastest-alone kernel forms, so they must give
the same bits; the same pair with a join in place of the loudness must agree in the formatted buffer, the layout record and the pauses record.
Measured on the commit before the chain was folded into one function: bit-equal in all of them (largest absolute difference 0), so equality is what is asserted."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_TOKENS = (12, 5, 9)


@pytest.fixture(scope="module")
def setup(dev):
    from chatterbox_amd import synth
    from chatterbox_amd.engine import S3GenEngine
    eng = S3GenEngine(synth.s3gen_state_dict(0), dev)
    eng._pipeline_streams()
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate(N_TOKENS)]
    # speeds at which rows 0 and 2 are longer than the meter's 0.4 s block; speed / 2^(pitch / 12) stays inside [0.5, 2]
    opts = dict(n_cfm_timesteps=2, seeds=[11, 12, 13], speed=[0.8, None, 0.5], pitch=[2, None, -3], pauses=dict(keep=[2, 0, 3], db=30),
                format=dict(sample_rate=8000, encoding="mulaw"))
    return eng, synth.s3gen_ref(), st, opts


def _same(a, b, what):
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    diff = (a.double() - b.double()).abs()
    print(f"{what}: {a.numel()} elements, {int((diff > 0).sum())} differ, largest absolute difference {float(diff.max()) if a.numel() else 0.0}")
    assert torch.equal(a, b), what


def test_rows_on_the_vocoder_stream_are_the_rows_of_the_default_stream(setup):
    from chatterbox_amd import ops
    eng, ref, st, opts = setup
    loud = [-16, None, -23]
    rows, _ = eng.vocode(st, ref, loudness=loud, **opts)
    stats, record = eng.last_loudness.clone(), eng.last_pauses.clone()
    res, _ = eng.vocode(st, ref, loudness=loud, hift_stream=eng._s_voc, sync=False, **opts)
    torch.cuda.synchronize()
    assert set(res) == {"rows", "pauses", "format"} and res["format"] == opts["format"]
    cut = ops.cut_pauses(res["rows"], res["pauses"].cpu(), res["format"])
    assert len(rows) == len(cut) == 3 and all(r.dtype == torch.uint8 and r.numel() > 0 for r in rows)
    for b, (x, y) in enumerate(zip(rows, cut)):
        _same(x, y, f"row {b}")
    _same(stats, eng.last_loudness, "loudness stats")
    _same(record, eng.last_pauses, "pauses record")


def test_joined_piece_on_the_vocoder_stream_is_the_piece_of_the_default_stream(setup):
    eng, ref, st, opts = setup
    join = dict(gaps=[480, 0, 240], trim_db=40.0)
    a, _ = eng.vocode(st, ref, join=join, **opts)
    b, _ = eng.vocode(st, ref, join=join, hift_stream=eng._s_voc, sync=False, **opts)
    torch.cuda.synchronize()
    assert a["format"] == b["format"] == opts["format"] and a["n"] == b["n"] and a["formatted"].dtype == torch.uint8
    for key in ("formatted", "rec", "pauses"):
        _same(a[key], b[key], key)
