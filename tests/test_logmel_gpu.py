"""GPU: Whisper log-mel features on the device (csrc/audio_features.hip through ops.logmel, LogMelEngine, the
WhisperFeatureExtractor drop-in, QwenOmniThinker(audio_waveforms=), SpiderFreeInfer(device_audio_features=True)) against the fp64
definition and against transformers' extractor. Clips, references and bounds: logmel_cases.py. Every case but one runs the small
configuration (n_samples 32000, cap 200).

Bounds: max |device - definition| <= 2^-13 on every element, max |device - HF| <= 2^-12 (logmel_cases.py says where they come from)."""
import numpy as np
import pytest
import torch

import logmel_cases as LC
from oracle import qwen_towers as oq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(dev):
    from spider_amd.audio_features import LogMelEngine
    return LogMelEngine(LC.SMALL, dev)


def _check(feat, mask, signal, L, what):
    host, hf, hf_mask, nv = LC.reference(signal, L)
    f = feat.cpu()
    e_host = float((f.double() - host).abs().max())
    e_hf = float((f - hf).abs().max())
    print(f"{what} {signal} L={L}: |device - definition| {e_host:.3e}  |device - HF| {e_hf:.3e}")
    assert e_host <= LC.TOL_HOST, f"{what} {signal} L={L}: {e_host:.3e} from the definition"
    assert e_hf <= LC.TOL_HF, f"{what} {signal} L={L}: {e_hf:.3e} from HF"
    assert mask.dtype == torch.int32 and torch.equal(mask.cpu(), hf_mask.to(torch.int32))
    tail = f[:, nv + 2:]
    if tail.numel():
        assert bool((tail == tail[0, 0]).all()), f"{what} {signal} L={L}: frames >= nv + 2 do not hold one value"
    return nv


@pytest.mark.parametrize("signal", LC.SIGNALS)
def test_every_length_of_a_signal_in_one_batch(engine, signal):
    """the 15 lengths as one packed batch: clip ends, hop / window boundaries, the tail reflect, truncation; offsets of every parity"""
    clips = [LC.clip(signal, L) for L in LC.LENGTHS]
    feat, mask, frames = engine(clips, 16000)
    assert tuple(feat.shape) == (len(clips), 128, 200) and feat.dtype == torch.float32 and feat.is_cuda
    for b, L in enumerate(LC.LENGTHS):
        assert frames[b] == _check(feat[b], mask[b], signal, L, "batch")
    if signal == "zeros":
        assert bool((feat == -1.5).all())


def test_single_clips_equal_the_batched_result(engine):
    """one clip per call (offset 0, the grid sized by that clip alone) gives the bits the batch of 15 gave"""
    clips = [LC.clip("chirp", L) for L in LC.LENGTHS]
    both = engine(clips)[0]
    for b, L in enumerate(LC.LENGTHS):
        if L in (1, 401, 32000, 40000):
            one, m, fr = engine([clips[b]])
            _check(one[0], m[0], "chirp", L, "single")
            assert torch.equal(one[0], both[b])


def test_batch_of_three_keeps_each_clips_maximum(engine):
    """a loud clip, an all-zero clip and a quiet one: the clip maximum (and with it clamp and floor) is per clip"""
    cases = [("clipped", 31999), ("zeros", 1000), ("tone440", 401)]
    feat, mask, frames = engine([LC.clip(s, L) for s, L in cases])
    for b, (s, L) in enumerate(cases):
        _check(feat[b], mask[b], s, L, "three")
    assert bool((feat[1] == -1.5).all())
    assert frames == [200, 7, 3] and mask.sum(1).tolist() == frames
    floors = [float(feat[b, 0, -1]) for b in range(3)]
    assert floors[1] == -1.5 and floors[2] != floors[1]            # the zero clip's floor did not leak into its neighbour


def test_float64_input_and_truncation_as_hf(engine):
    x = LC.clip("noise", 40000)
    a = engine([x.astype(np.float64)])[0]
    b = engine([torch.from_numpy(x.copy())[:32000]])[0]
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="sampling rate"):
        engine([x], 8000)


def test_runs_are_bit_identical_and_a_graph_replay_equals_eager(engine, dev):
    from spider_amd import ops
    clips = [LC.clip("noise", 31999), LC.clip("bursts", 1000), LC.clip("chirp", 401)]
    waves, meta, lens = engine.pack(clips)
    run = lambda out=None, mask=None: ops.logmel(waves, lens, engine.tables, out=out, mask=mask, offsets=meta[0], lengths_dev=meta[1])
    f1, m1 = run()
    f2, m2 = run()
    assert torch.equal(f1, f2) and torch.equal(m1, m2)
    out, mask = torch.full_like(f1, float("nan")), torch.full_like(m1, -1)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            run(out, mask)
    torch.cuda.current_stream().wait_stream(s)
    out.fill_(float("nan")); mask.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, f1) and torch.equal(mask, m1)
    # ops.logmel builds the device arrays itself from the host lengths: the same result
    f3, m3 = ops.logmel(waves, lens, engine.tables)
    assert torch.equal(f3, f1) and torch.equal(m3, m1)


def test_full_cap_configuration_three_seconds_of_noise(dev):
    """Qwen2.5-Omni's own configuration (n_samples 4.8 M, cap 30000), B = 1, 3 s of noise: 302 frames computed, floor fill and mask
    over the whole array, against the definition and HF's extractor at chunk_length 300."""
    from spider_amd.audio_features import LogMelConfig, LogMelEngine, logmel_host
    cfg = LogMelConfig()
    x = LC.clip("noise", 48000)
    feat, mask, frames = LogMelEngine(cfg, dev)([x], 16000)
    assert tuple(feat.shape) == (1, 128, 30000) and tuple(mask.shape) == (1, 30000) and frames == [300]
    hf, hf_mask = LC.hf_call([x], chunk_length=300)
    f = feat[0].cpu()
    host = logmel_host(x, cfg)
    e_host, e_hf = float((f.double() - host).abs().max()), float((f - hf[0]).abs().max())
    print(f"full cap: |device - definition| {e_host:.3e}  |device - HF| {e_hf:.3e}")
    assert e_host <= LC.TOL_HOST and e_hf <= LC.TOL_HF
    assert torch.equal(mask[0].cpu(), hf_mask[0].to(torch.int32)) and int(mask.sum()) == 300
    assert bool((f[:, 302:] == f[0, 302]).all())


def test_torch_op_equals_ops_logmel(engine, dev):
    import spider_amd.torch_ops as T
    from spider_amd import ops
    assert T.AUDIO_OP_NAMES == ("logmel",) and hasattr(torch.ops.spider_hip, "logmel")
    clips = [LC.clip("noise", 1000), LC.clip("tone1k", 401)]
    waves, meta, lens = engine.pack(clips)
    t = engine.tables
    f, m = torch.ops.spider_hip.logmel(waves, meta[0], meta[1], max(lens), t["table"], t["fb"], t["n_samples"], t["hop"])
    ref_f, ref_m = ops.logmel(waves, lens, t)
    assert torch.equal(f, ref_f) and torch.equal(m, ref_m)


# ---------------------------------------------------------------------------------------------- plumbing (exact)
def test_drop_in_answers_the_processors_call_like_hf(dev):
    from spider_amd.audio_features import DeviceWhisperFeatureExtractor
    fe = LC.hf_extractor(2)
    dfe = DeviceWhisperFeatureExtractor.from_feature_extractor(fe, dev)
    clips = [LC.clip("noise", 1000), LC.clip("chirp", 32000)]
    kw = dict(sampling_rate=16000, padding="max_length", return_attention_mask=True, return_tensors="pt")
    got, ref = dfe(clips, **kw), fe([np.asarray(c) for c in clips], **kw)
    assert type(got) is type(ref) and set(got.keys()) == set(ref.keys()) == {"input_features", "attention_mask"}
    for k in ref.keys():
        assert got[k].is_cuda and got[k].dtype == ref[k].dtype and tuple(got[k].shape) == tuple(ref[k].shape), k
    assert torch.equal(got["attention_mask"].cpu(), ref["attention_mask"])
    assert float((got["input_features"].cpu() - ref["input_features"]).abs().max()) <= LC.TOL_HF
    single = dfe(clips[0], **kw)                                   # one clip, not a list: still a batch of one
    assert tuple(single["input_features"].shape) == (1, 128, 200) and torch.equal(single["input_features"][0], got["input_features"][0])
    assert set(dfe(clips, sampling_rate=16000, return_tensors="pt").keys()) == {"input_features"}
    for bad in (dict(padding="longest"), dict(padding=True), dict(truncation=False), dict(max_length=16000), dict(do_normalize=True),
                dict(return_tensors="np")):
        with pytest.raises(NotImplementedError):
            dfe(clips, **dict(kw, **bad))
    with pytest.raises(ValueError):
        dfe(clips, **dict(kw, sampling_rate=22050))


def _tiny_thinker(dev, seed=7):
    from oracle.llama import LlamaCfg, LlamaOracle
    from spider_amd.audio_features import LogMelConfig, LogMelEngine
    from spider_amd.llm import LlamaEngine, LLMConfig
    from spider_amd.qwen_omni import AudioTowerConfig, AudioTowerEngine, OmniTokenIds, QwenOmniThinker
    H = 256
    lcfg = LlamaCfg(H, 2, 4, 2, 128, 512, 400, 1000000.0, None, 1e-6, True, 512, False, (16, 24, 24))
    lw = LlamaOracle.random_weights(lcfg, seed=seed, std=0.08)
    ac = oq.AudioCfg(mel=16, layers=2, heads=2, ffn=96, d_model=32, max_pos=40, n_window=10, out_dim=H)
    aw = oq.random_weights(oq.audio_param_shapes(ac), seed=seed + 2)
    tok = OmniTokenIds(image=390, video=391, audio=392, vision_start=393, audio_start=394)
    logmel = LogMelEngine(LogMelConfig(feature_size=16, chunk_length=2), dev)
    th = QwenOmniThinker(LlamaEngine(LLMConfig(**lcfg.__dict__), lw, dev, max_batch=1, max_len=128), None,
                         AudioTowerEngine(AudioTowerConfig(**ac.__dict__), aw, dev), tok, logmel=logmel)
    return th, logmel


def _audio_prompt(frames):
    return [5, 6, 394] + [392] * sum(oq.audio_output_lengths(frames)) + [395, 7, 8, 9]


def test_thinker_audio_waveforms_equal_the_feature_path_bit_for_bit(dev):
    th, logmel = _tiny_thinker(dev)
    clips = [LC.clip("noise", 47 * 160 - 30), LC.clip("chirp", 21 * 160)]          # 47 and 21 mel frames
    F, M, frames = logmel(clips, 16000)
    assert frames == [47, 21]
    ids = torch.tensor([_audio_prompt(frames)])
    e_ref, p_ref = th.prepare_inputs(ids, torch.ones_like(ids), input_features=F, feature_attention_mask=M)
    e, p = th.prepare_inputs(ids, torch.ones_like(ids), audio_waveforms=clips, sampling_rate=16000)
    assert torch.equal(e, e_ref) and torch.equal(p, p_ref)
    kw = dict(max_new_tokens=4, eos_token_id=[])
    assert torch.equal(th.generate(ids, None, audio_waveforms=clips, **kw), th.generate(ids, None, input_features=F, feature_attention_mask=M, **kw))
    # the tower graph of these lengths exists now: the answer is the feature path's; another length would capture
    assert th.would_capture(ids, audio_waveforms=clips) == th.would_capture(ids, input_features=F, feature_attention_mask=M)
    assert th.would_capture(ids, audio_waveforms=[clips[0][:1600]]) is True
    with pytest.raises(ValueError, match="not both"):
        th.prepare_inputs(ids, None, audio_waveforms=clips, input_features=F, feature_attention_mask=M)
    with pytest.raises(ValueError, match="sampling rate"):
        th.prepare_inputs(ids, None, audio_waveforms=clips, sampling_rate=8000)


def test_spider_free_infer_with_a_clip_in_the_request(dev):
    """SpiderFreeInfer(device_audio_features=True): the processor's WhisperFeatureExtractor is swapped for the drop-in once, a request
    that carries a clip is answered with the tokens the thinker generates from the waveform; with the flag off nothing is swapped."""
    from transformers import WhisperFeatureExtractor
    from benchkit.synthetic import SyntheticOmniProcessor
    from spider_amd import SpiderDecoderInfer, SpiderFreeInfer
    from spider_amd.audio_features import DeviceWhisperFeatureExtractor
    th, _ = _tiny_thinker(dev, seed=27)
    clip = LC.clip("bursts", 47 * 160)
    ids = torch.tensor([_audio_prompt([47])])

    class Proc(SyntheticOmniProcessor):          # what Qwen2_5OmniProcessor does with one clip: placeholders + its feature extractor's output
        def __init__(self, **kw):
            super().__init__(**kw)
            self.feature_extractor = WhisperFeatureExtractor(feature_size=16, n_fft=400, hop_length=160, chunk_length=2)

        def __call__(self, text=None, audios=None, images=None, videos=None, return_tensors="pt", padding=True):
            self.prompt_len = ids.shape[1]
            out = {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
            if audios is not None:
                a = self.feature_extractor(audios, sampling_rate=16000, padding="max_length", return_attention_mask=True, return_tensors="pt")
                out.update(input_features=a["input_features"], feature_attention_mask=a["attention_mask"])
            return out

    class Pipe:
        def __call__(self, prompt=None, **kw):
            class O:
                images = [f"img:{p}" for p in prompt]
            return O()

    mk = lambda: SpiderDecoderInfer({"model": dict(type="spider_decoder", pipelines={"IMAGE": Pipe()}, device=str(dev))})
    gk = dict(max_new_tokens=6, eos_token_id=[], spk="Chelsie", use_audio_in_video=True)
    mm = lambda messages, use_audio_in_video: ([clip], None, None)
    off_proc = Proc(vocab=400)
    fe = off_proc.feature_extractor
    off = SpiderFreeInfer(th, off_proc, mk(), device=dev, generate_kwargs=gk, process_mm_info=mm)
    assert off_proc.feature_extractor is fe
    on_proc = Proc(vocab=400)
    on = SpiderFreeInfer(th, on_proc, mk(), device=dev, generate_kwargs=gk, process_mm_info=mm, device_audio_features=True)
    assert isinstance(on_proc.feature_extractor, DeviceWhisperFeatureExtractor) and on_proc.feature_extractor.feature_size == 16
    msgs = [{"role": "user", "content": [{"type": "audio", "audio": "x.wav"}, {"type": "text", "text": "what do you hear?"}]}]
    res = on(msgs)
    direct = th.generate(ids, None, max_new_tokens=6, eos_token_id=[], audio_waveforms=[clip], sampling_rate=16000)
    assert torch.equal(res.text_ids, direct[0].cpu()), "the request is answered from the device features of its clip"
    assert res.predictions["IMAGE"] == [f"img:{res.predictions_text['IMAGE'][0]}"]
    inputs = on.build_inputs(msgs)
    assert inputs["input_features"].is_cuda and inputs["feature_attention_mask"].is_cuda
    assert not off.build_inputs(msgs)["input_features"].is_cuda
    with pytest.raises(ValueError, match="WhisperFeatureExtractor"):
        SpiderFreeInfer(th, SyntheticOmniProcessor(vocab=400), mk(), device=dev, device_audio_features=True)
