"""`IndexTTS` drop-in (/root/reference/indextts/infer.py:25-537) on the MI355X HIP engine.

Same constructor and methods (`extract_features`, `infer`, `infer_fast`, `set_gr_progress_callback`,
`remove_long_silence`, `bucket_sentences`, `pad_tokens_cat`), same attributes (`device`, `cfg`, `tokenizer`,
`gpt`, `bigvgan`, `stop_mel_token`).  Differences, all deliberate:
  * `infer` accepts this fork's `prompt_mel=<tensor [1,100,F]>` AND upstream's `audio_prompt=<wav path>` (the
    reference's own cli.py:70 and tests call the latter, which this fork's signature rejects);
  * conditioning latents and the ECAPA speaker vector are computed once per prompt and reused across sentences;
  * `infer` decodes the sentences of a text in batches of up to max_batch rows (the reference loops at batch 1; rows of a
    batch are independent), `infer_fast` in the reference's length-sorted buckets; both vocode as the reference does
    (`infer` per sentence, `infer_fast` over time-concatenated chunks of 2 latents); `infer_batch` takes several utterances;
  * every public call takes the engine lock: several host threads may share one IndexTTS (webui.py:441-452);
  * generation runs on the device for every mode the kwargs of infer.py:116-124 select: beam-sample (the default:
    do_sample=True, num_beams=3; up to 10 beams, per-beam cache ancestry instead of HF's per-step cache copy), beam search
    (do_sample=False, num_beams > 1), multinomial sampling (num_beams=1) and greedy - with top_k <= 128 / top_p /
    temperature / repetition_penalty / length_penalty and `typical_sampling` (TypicalLogitsWarper) in HF 4.36.2 semantics;
    `top_k = 0 / None` (HF: TopK warper off) or > 128 is exact too, with one beam or several - the warpers and draws then run on
    the host over the whole vocabulary, one logits read-back per token (under beams BeamSearchScorer.process, the beam
    re-ordering and finalize stay on the device).
    Draws come from a numpy Generator seeded from torch's global RNG, so `torch.manual_seed` makes a run reproducible
    (torch.multinomial's own stream cannot be reproduced on a device);
  * the text normaliser is built and loaded as in infer.py:69-71; its third-party written-form normalisers (`tn` /
    `wetext`) are used when installed and skipped with a RuntimeWarning otherwise (punctuation folding, pinyin and name
    protection always apply);
  * `is_fp16=True` selects the IEEE-half engine (the reference's own GPU precision; ITTS_HALF=bf16: the bfloat16 engine, same
    speed), `False` the fp32 parity engine; `use_cuda_kernel` is accepted
    and ignored (the fused HIP activation is always used);
  * `gpt_fp8=True` (not in the reference; needs `is_fp16=True`) stores the GPT projections and mel_head as fp8-e4m3 with
    power-of-two row scales (pack.quantize_gpt_fp8), runs on the bfloat16 engine - the fp8 readers expand to bf16 pairs - and
    lets the 1 - 6 row decode steps stream the fp8 bytes on the persistent decode engine.
  * `kv_fp8=True` (not in the reference; needs `is_fp16=True`, works with both 16-bit engines and together with `gpt_fp8`) keeps
    the K/V cache of the GPT decode steps as fp8-e4m3 bytes: half the cache bytes per step; the decode steps keep the launch path.
  * `engine_kv_fp8=True` (not in the reference; needs `kv_fp8=True`, ValueError otherwise) keeps the 1 - 6 row decode steps of an
    fp8-cache generation on the persistent decode engine, which reads and appends the e4m3 rows itself.
  * `retire_rows=r` (not in the reference; a ratio in (0, 1], None: ITTS_RETIRE_ROWS, else off) lets the batched generations
    of `infer_fast` / `infer_batch` retire their finished rows: whenever the unfinished rows are <= r * the running rows (and more
    than 6 rows run), the decode state is compacted and the following steps run at the smaller row count (Engine.generate).
  * `retire_beams=True` (not in the reference; None: ITTS_RETIRE_BEAMS, else off; acts only together with `retire_rows`) extends
    the row retirement to the beam generations - the mode of the default kwargs, `num_beams=3`: a finished sentence's group of
    `num_beams` rows is retired as a unit and its hypotheses are kept by sentence (Engine.generate(retire_beams=..)).
  * `ragged_vocoder=True` (not in the reference; default off; ITTS_RAGGED_VOCODER=1 / 0 overrides it in both directions) lets the
    sentences of `infer_batch` share vocoder passes although their lengths differ (Engine.bigvgan_grouped(ragged=True)); without
    it only sentences of equal length do.  `infer` / `infer_fast` are not affected.
  * `mixed_batch=True` (not in the reference; default off; ITTS_MIXED_BATCH=1 / 0 overrides it in both directions) lets the
    utterances of one `infer_batch` call share decode batches across voices and - with one beam and no typical filter - across
    sampling settings (`per_utterance`): conditioning and the speaker encoder run once per distinct prompt, every decode row
    carries its own conditioning latents and its own do_sample / top_k / top_p / temperature / repetition_penalty / seed, the
    latent pass and the vocoder take one voice per sentence.  `infer` / `infer_fast` are not affected.
  * `admit_rows=True` (not in the reference; default off; ITTS_ADMIT_ROWS=1 / 0 overrides it in both directions; needs
    `mixed_batch`, without which it does nothing and says so once) lets a group of `infer_batch` with more sentences than
    `max_batch` decode as ONE generation of `max_batch` rows: a finished row's slot takes the next waiting sentence
    (Engine.generate(slots=..)) instead of every `max_batch`-sized generation draining to its slowest row.  Single beam, no
    typical filter, more than 6 rows.  `infer` / `infer_fast` are not affected.
  * `admit_beams=True` (not in the reference; default off; ITTS_ADMIT_BEAMS=1 / 0 overrides it in both directions; acts only on top
    of `admit_rows` + `mixed_batch`) extends the row admission to the beam groups of `infer_batch` - the mode of the default
    kwargs, `num_beams=3` - without typical filtering: a group with more sentences than `max_batch // num_beams` decodes as ONE
    generation of that many item slots, a finished sentence's group of `num_beams` rows takes the next waiting sentence
    (Engine.generate(slots=.., admit_beams=True)).  `infer` / `infer_fast` and plain `infer_batch` are not affected.
  * `packed_latent=True` (not in the reference; default off; ITTS_PACKED_LATENT=1 / 0 overrides it in both directions) runs the
    latent pass of `infer_batch` on packed rows (Engine.latent_packed: no pad rows, a sentence's latent has the same bits
    whoever shares its pass); with `mixed_batch` the utterances of a decode group then share ONE latent pass instead of one
    per utterance.  The vocoder stays per utterance unless `packed_vocoder` is on.  `infer` / `infer_fast` are not affected.
  * `packed_vocoder=True` (not in the reference; default off; ITTS_PACKED_VOCODER=1 / 0 overrides it in both directions) runs the
    vocoder of `infer_batch` over its sentences back to back as one item (Engine.bigvgan_packed: no padding to a common length, a
    sentence's waveform has the same bits whoever shares its pass) where it otherwise calls Engine.bigvgan_grouped; with
    `mixed_batch` the utterances and voices of a decode group then share ONE vocoder pass instead of one set of passes per
    utterance.  It takes precedence over `ragged_vocoder`.  `infer` / `infer_fast` are not affected.
  * `infer_stream(...)` (not in the reference) is `infer` as a GENERATOR of (24000, int16 [n, 1]) chunks: a sentence's
    audio starts to arrive while its codes are still being decoded.  One beam only.  `stream_chunk_frames=N` holds the default
    chunk size in latent frames (ITTS_STREAM_CHUNK overrides it).  `infer` / `infer_fast` / `infer_batch` are not affected.
There is no CPU fallback: without a GPU / libitts_hip.so construction raises."""
from __future__ import annotations

import os
import time
import warnings
from typing import List

import numpy as np
import torch

from itts_hip import config as icfg
from itts_hip import engine as ieng
from itts_hip import infer_core, pack
from indextts.BigVGAN.models import BigVGAN as Generator
from indextts.gpt.model import UnifiedVoice
from indextts.utils.checkpoint import read_state_dict
from indextts.utils.feature_extractors import MelSpectrogramFeatures, load_wav_mono, resample
from indextts.utils.front import TextNormalizer, TextTokenizer


class IndexTTS:
    def __init__(self, cfg_path="checkpoints/config.yaml", model_dir="checkpoints", is_fp16=True, device=None,
                 use_cuda_kernel=None, state_dicts=None, cfg=None, gpt_fp8=False, wide_sampler=None,
                 wide_beam_sampler=None, kv_fp8=False, retire_rows=None, engine_kv_fp8=False, ragged_vocoder=False,
                 mixed_batch=False, admit_rows=False, retire_beams=None, packed_latent=False, admit_beams=False,
                 packed_vocoder=False, stream_chunk_frames=None):
        # fp8 K/V cache on the persistent decode engine: a mode of the fp8 cache (checked before anything touches the device)
        self.engine_kv_fp8 = bool(engine_kv_fp8)
        if self.engine_kv_fp8 and not kv_fp8:
            raise ValueError("engine_kv_fp8=True needs kv_fp8=True: it keeps the fp8 K/V cache's small-batch decode steps on the "
                             "persistent decode engine and has no effect on the 16-bit cache")
        if device is None:
            device = "cuda:0"
        if not str(device).startswith("cuda") or not torch.cuda.is_available():
            raise RuntimeError("IndexTTS (itts_hip): an MI355X GPU is required; there is no CPU fallback")
        self.device = str(device)
        self.is_fp16 = bool(is_fp16)
        self.use_cuda_kernel = True
        self.cfg = cfg if cfg is not None else icfg.load_yaml(cfg_path)
        self.model_dir = model_dir
        # is_fp16=True is IEEE half in the reference (autocast(dtype=torch.float16) + .half(), infer.py:39,44,52): the f16 build of the
        # library.  ITTS_HALF=bf16 selects the bfloat16 engine instead (same speed, 8 instead of 11 significand bits, wider range)
        self.half = os.environ.get("ITTS_HALF", "bf16" if gpt_fp8 else "f16") if self.is_fp16 else None
        if self.half not in (None, "f16", "bf16"):
            raise ValueError(f"ITTS_HALF={self.half}: expected f16 or bf16")
        # gpt_fp8: fp8-e4m3 GPT weights.  The fp8 readers expand to bf16 pairs, so it is a mode of the bfloat16 engine only
        self.gpt_fp8 = bool(gpt_fp8)
        # how do_sample with one beam and top_k = 0 / None or > 128 runs: "host" (torch's arithmetic, one sync per token), "device"
        # (the whole-vocabulary device sampler), None: ITTS_WIDE_SAMPLER, else "host" (Engine.generate)
        self.wide_sampler = wide_sampler
        # the same choice for several beams (beam_sample with top_k = 0 / None or > 128): None: ITTS_WIDE_BEAM_SAMPLER, else "host"
        self.wide_beam_sampler = wide_beam_sampler
        self.retire_rows = retire_rows  # row retirement of the batched generations (Engine.generate); None: ITTS_RETIRE_ROWS, else off
        self.retire_beams = retire_beams  # with retire_rows: beam generations retire their finished groups; None: ITTS_RETIRE_BEAMS, else off
        self.ragged_vocoder = bool(ragged_vocoder)  # infer_batch: sentences of unequal length share vocoder passes (ITTS_RAGGED_VOCODER overrides)
        self.mixed_batch = bool(mixed_batch)  # infer_batch: one decode batch across voices and sampling settings (ITTS_MIXED_BATCH overrides)
        self.admit_rows = bool(admit_rows)  # infer_batch with mixed_batch: finished decode rows are refilled from the waiting sentences (ITTS_ADMIT_ROWS overrides)
        self.admit_beams = bool(admit_beams)  # on top of admit_rows: beam groups (the default kwargs' mode) are refilled too (ITTS_ADMIT_BEAMS overrides)
        self._admit_told = False
        self.packed_latent = bool(packed_latent)  # infer_batch: the latent pass on packed rows, one per decode group (ITTS_PACKED_LATENT overrides)
        self.packed_vocoder = bool(packed_vocoder)  # infer_batch: the vocoder over sentences back to back, one pass per decode group (ITTS_PACKED_VOCODER overrides)
        # infer_stream: latent frames per audio chunk (1 frame = 1024 samples); None: infer_core.STREAM_CHUNK_FRAMES; ITTS_STREAM_CHUNK overrides
        self.stream_chunk_frames = None if stream_chunk_frames is None else max(1, int(stream_chunk_frames))
        self.kv_fp8 = bool(kv_fp8)  # fp8-e4m3 K/V cache of the decode steps: either 16-bit engine
        if self.kv_fp8 and not self.is_fp16:
            raise ValueError("kv_fp8=True needs is_fp16=True: the fp8 K/V cache is a mode of the 16-bit engines, not the fp32 one")
        if self.gpt_fp8 and not self.is_fp16:
            raise ValueError("gpt_fp8=True needs is_fp16=True: the fp8 GPT weights run on the bfloat16 engine, not the fp32 one")
        if self.gpt_fp8 and self.half != "bf16":
            raise ValueError("gpt_fp8=True needs the bfloat16 engine: fp8 weights expand to bf16 pairs (unset ITTS_HALF=f16)")
        self.dtype = (torch.float16 if self.half == "f16" else torch.bfloat16) if self.is_fp16 else torch.float32
        self.stop_mel_token = self.cfg.gpt.stop_mel_token
        sds = dict(state_dicts or {})
        if "gpt" not in sds:
            self.gpt_path = os.path.join(model_dir, self.cfg.gpt_checkpoint)
            sds["gpt"] = read_state_dict(self.gpt_path)
            print(">> GPT weights restored from:", self.gpt_path)
        if "bigvgan" not in sds:
            self.bigvgan_path = os.path.join(model_dir, self.cfg.bigvgan_checkpoint)
            sds["bigvgan"] = read_state_dict(self.bigvgan_path, key="generator")
            print(">> bigvgan weights restored from:", self.bigvgan_path)
        self.engine = ieng.Engine(self.cfg, self.half if self.is_fp16 else "fp32", self.device)
        packed_gpt = pack.pack_gpt(sds["gpt"], self.cfg)
        if self.gpt_fp8:
            packed_gpt = pack.quantize_gpt_fp8(packed_gpt, keep_bytes=True)
        self.engine.load_packed(packed_gpt)
        self.engine.load_packed(pack.pack_bigvgan(sds["bigvgan"], self.cfg))
        if "dvae" in sds:
            self.engine.load_packed(pack.pack_dvae(sds["dvae"], self.cfg))
        self.engine.finalize()
        if self.gpt_fp8:
            self.engine.set_engine_fp8(True)
        if self.kv_fp8:
            self.engine.set_kv_fp8(True)
        if self.engine_kv_fp8:
            self.engine.set_engine_kv_fp8(True)
        self.gpt =UnifiedVoice(self.engine, self.cfg.gpt)
        self.bigvgan = Generator(self.engine)
        self.bpe_path = os.path.join(model_dir, self.cfg.dataset["bpe_model"])
        self.normalizer = TextNormalizer()  # infer.py:69-71
        self.normalizer.load()
        self.tokenizer = TextTokenizer(self.bpe_path, self.normalizer)
        print(">> bpe model loaded from:", self.bpe_path)
        self.wav2mel = MelSpectrogramFeatures()
        self.gr_progress = None

    def set_gr_progress_callback(self, _callback):
        self.gr_progress = _callback

    def _set_gr_progress(self, value, desc):
        if self.gr_progress is not None:
            self.gr_progress(value, desc)

    def extract_features(self, audio_prompt_path: str) -> torch.Tensor:
        """wav path -> log-mel [1, 100, F] on the device (infer.py:82-93)."""
        audio, sr = load_wav_mono(audio_prompt_path)
        audio = resample(audio, sr, 24000)
        return self.wav2mel(audio).to(self.device)

    # ---- integer host logic (infer.py:244-318) ----
    def remove_long_silence(self, codes: torch.Tensor, silent_token=52, max_consecutive=30):
        c, n = infer_core.remove_long_silence(codes.detach().cpu().numpy(), self.stop_mel_token, silent_token, max_consecutive)
        return torch.from_numpy(c).to(codes.device), torch.from_numpy(n).to(codes.device)

    def bucket_sentences(self, sentences, bucket_max_size=4):
        return infer_core.bucket_sentences(sentences, bucket_max_size)

    def pad_tokens_cat(self, tokens: List[torch.Tensor]) -> torch.Tensor:
        arr = infer_core.pad_tokens_cat([t.detach().cpu().numpy() for t in tokens], self.cfg.gpt.stop_text_token)
        return torch.from_numpy(arr).to(self.device)

    def torch_empty_cache(self):
        torch.cuda.empty_cache()

    # ---- synthesis ----
    def _sentences_to_ids(self, text, max_tokens):
        if isinstance(text, str):
            toks = self.tokenizer.tokenize(text)
            sents = self.tokenizer.split_sentences(toks, max_tokens)
            return [np.asarray(self.tokenizer.convert_tokens_to_ids(s), dtype=np.int32) for s in sents]
        return [np.asarray(s, dtype=np.int32).reshape(-1) for s in text]  # pre-tokenised: list of id lists

    def _gen_kwargs(self, kw):
        """The generation kwargs `infer` / `infer_fast` pop (infer.py:116-124), with the reference's defaults."""
        kw = dict(kw)
        g = dict(do_sample=kw.pop("do_sample", True), top_p=kw.pop("top_p", 0.8), top_k=kw.pop("top_k", 30),
                 temperature=kw.pop("temperature", 1.0), length_penalty=kw.pop("length_penalty", 0.0),
                 num_beams=kw.pop("num_beams", 3), repetition_penalty=kw.pop("repetition_penalty", 10.0),
                 max_mel_tokens=kw.pop("max_mel_tokens", 600))
        g["typical_sampling"] = kw.pop("typical_sampling", False)
        g["typical_mass"] = kw.pop("typical_mass", 0.9)
        return g

    def _generate_rows(self, cond, sents, g):
        """Mel codes for a list of sentences: decode batches of at most `engine max_batch` rows (HF pads / stops per
        batch, so a group is exactly one `inference_speech` call of the reference)."""
        sample_kw = infer_core.sampling_kwargs(g["do_sample"], g["num_beams"], g["top_k"], g["top_p"], g["temperature"],
                                               g["typical_sampling"], g["typical_mass"], g["length_penalty"])
        if g.get("seed") is not None and "seed" in sample_kw:
            sample_kw["seed"] = int(g["seed"])  # infer_batch(per_utterance=[{"seed": ..}]): the caller's seed instead of a drawn one
        cap = max(1, self.engine.ccfg.max_batch // max(1, sample_kw.get("num_beams", 1)))
        rows = []
        for lo in range(0, len(sents), cap):
            grp = sents[lo:lo + cap]
            ids = infer_core.pad_tokens_cat(grp, self.cfg.gpt.stop_text_token)
            codes = self.engine.generate(cond, ids, g["max_mel_tokens"], repetition_penalty=g["repetition_penalty"],
                                         wide_sampler=self.wide_sampler, wide_beam_sampler=self.wide_beam_sampler,
                                         retire_rows=self.retire_rows, retire_beams=self.retire_beams, **sample_kw)
            rows.extend(codes[r] for r in range(len(grp)))
        return rows

    def _clean_and_latents(self, cond, sents, code_rows, max_mel_tokens, packed=False):
        """remove_long_silence per sentence (infer.py:190 / :463), then the latent pass (batch-1 semantics per sentence,
        stacked as masked left-padded rows in one launch sequence; packed: as packed rows, Engine.latent_packed)."""
        if any(r[-1] != self.stop_mel_token for r in code_rows):
            warnings.warn(f"WARN: generation stopped due to exceeding `max_mel_tokens` ({max_mel_tokens}). "
                          "Consider reducing `max_text_tokens_per_sentence` or increasing `max_mel_tokens`.", RuntimeWarning)
        clean = []
        for r in code_rows:
            c, n = infer_core.remove_long_silence(np.asarray(r)[None], self.stop_mel_token)
            clean.append(c[0, : int(n[0])])
        if packed:
            return self.engine.latent_packed(cond, sents, clean)
        lats = []
        cap = self.engine.ccfg.max_batch
        for lo in range(0, len(sents), cap):
            lats.extend(self.engine.latent_batch(cond, sents[lo:lo + cap], clean[lo:lo + cap]))
        return lats

    def _finish(self, wavs, output_path, start, timers, verbose, tag=""):
        wav = torch.cat(wavs, dim=1)
        total = time.perf_counter() - start
        wav_len = wav.shape[-1] / 24000
        if verbose:
            print(f">> gpt_gen_time: {timers[0]:.2f}s  gpt_forward_time: {timers[1]:.2f}s  bigvgan_time: {timers[2]:.2f}s")
        print(f">> Total {tag}inference time: {total:.2f} seconds; generated audio: {wav_len:.2f} s; RTF: {total / max(wav_len, 1e-9):.4f}")
        wav16 = wav.type(torch.int16)
        if output_path:
            from scipy.io import wavfile

            if os.path.isfile(output_path):
                os.remove(output_path)
            if os.path.dirname(output_path):
                os.makedirs(os.path.dirname(output_path), exist_ok=True)
            wavfile.write(output_path, 24000, wav16.numpy().T)
            return output_path
        return (24000, wav16.numpy().T)

    def _to_int16_range(self, wav):
        return torch.clamp(32767 * wav.squeeze(1), -32767.0, 32767.0).cpu()  # infer.py:208-212

    def _synthesize(self, prompt_mel, text, output_path, max_text_tokens_per_sentence, bucket, verbose, kw, fast):
        """`infer` (fast=False: vocoder per sentence, infer.py:134-212) and `infer_fast` (fast=True: length-sorted buckets
        for the AR decode, vocoder over time-concatenated chunks of 2 latents, infer.py:385-498)."""
        start = time.perf_counter()
        g = self._gen_kwargs(kw)
        sents = self._sentences_to_ids(text, max_text_tokens_per_sentence)
        if not sents:
            # the reference ends in torch.cat([]) -> RuntimeError; same class, clearer message
            raise RuntimeError("IndexTTS: the text produced no sentences (empty input)")
        self._set_gr_progress(0.1, "text processing...")
        with self.engine.lock:
            # the speaker embedding (needed by the vocoder only) on the engine's side stream, beside the conditioning encoder and the prefill
            spk = self.engine.ecapa(prompt_mel.transpose(1, 2), overlap=True)
            cond = self.gpt.get_conditioning(prompt_mel)
            t_gen = t_fwd = t_voc = 0.0
            t0 = time.perf_counter()
            code_rows = [None] * len(sents)
            if fast:
                for bk in infer_core.bucket_sentences(sents, bucket):
                    for item, row in zip(bk, self._generate_rows(cond, [x["sent"] for x in bk], g)):
                        code_rows[item["idx"]] = row
            else:
                code_rows = self._generate_rows(cond, sents, g)
            t_gen = time.perf_counter() - t0
            self._set_gr_progress(0.5, "gpt inference latents...")
            t0 = time.perf_counter()
            lats = self._clean_and_latents(cond, sents, code_rows, g["max_mel_tokens"])  # original sentence order
            t_fwd = time.perf_counter() - t0
            self._set_gr_progress(0.7, "bigvgan decode...")
            t0 = time.perf_counter()
            wavs = []
            if fast:
                chunk = 2  # infer.py:480: BigVGAN runs over pairs of sentences concatenated along time
                for lo in range(0, len(lats), chunk):
                    wavs.append(self._to_int16_range(self.engine.bigvgan(torch.cat(lats[lo:lo + chunk], dim=1), spk)))
            else:
                for lat in lats:
                    wavs.append(self._to_int16_range(self.engine.bigvgan(lat, spk)))
            t_voc = time.perf_counter() - t0
        self._set_gr_progress(0.9, "save audio...")
        return self._finish(wavs, output_path, start, (t_gen, t_fwd, t_voc), verbose, "fast " if fast else "")

    @torch.no_grad()
    def infer_batch(self, prompt_mels, texts, output_paths=None, max_text_tokens_per_sentence=120, verbose=False,
                    per_utterance=None, **generation_kwargs):
        """Several utterances in one call (the multi-utterance / data-parallel entry point): the sentences of
        all utterances that share a prompt are decoded together in length-sorted batches of up to `max_batch` rows,
        the latent pass is stacked, the vocoder runs per sentence.  Under torch.distributed (one process per GPU) each
        rank should pass its own shard - see itts_hip.dp.run_sharded.  prompt_mels: one tensor for all utterances or a
        list with one per utterance.  Returns a list of (24000, int16 [n, 1]) or of written paths.
        per_utterance (optional): a list with one dict of generation kwargs per utterance, on top of **generation_kwargs
        (plus `seed`: the seed of that utterance's draws instead of one drawn from torch's global RNG).  Utterances then run in
        groups of equal settings per prompt - or, with mixed_batch on, share decode batches across prompts and settings
        (_infer_batch_mixed)."""
        n = len(texts)
        prompts = [prompt_mels] * n if isinstance(prompt_mels, torch.Tensor) else list(prompt_mels)
        assert len(prompts) == n and (output_paths is None or len(output_paths) == n)
        assert per_utterance is None or len(per_utterance) == n
        settings = []
        for u in range(n):
            over = dict(per_utterance[u] or {}) if per_utterance is not None else {}
            seed = over.pop("seed", None)
            settings.append(dict(self._gen_kwargs(dict(generation_kwargs, **over)), seed=seed))
        start = time.perf_counter()
        utt_sents = [self._sentences_to_ids(t, max_text_tokens_per_sentence) for t in texts]
        results = [None] * n
        admit = {"1": True, "0": False}.get(os.environ.get("ITTS_ADMIT_ROWS", ""), self.admit_rows)
        if {"1": True, "0": False}.get(os.environ.get("ITTS_MIXED_BATCH", ""), self.mixed_batch):
            with self.engine.lock:
                self._infer_batch_mixed(prompts, utt_sents, settings, results, admit)
            groups = {}
        else:
            if admit and not self._admit_told:
                self._admit_told = True
                warnings.warn("admit_rows / ITTS_ADMIT_ROWS does nothing without mixed_batch / ITTS_MIXED_BATCH: row admission runs "
                              "on the per-row path of infer_batch only", RuntimeWarning)
            groups = {}  # utterances of one prompt and one setting, in the order of their first utterance
            for u, p in enumerate(prompts):
                groups.setdefault((id(p), tuple(sorted(settings[u].items(), key=lambda kv: kv[0]))), []).append(u)
        with self.engine.lock:
            for us in groups.values():
                g = settings[us[0]]
                mel = self._prompt(prompts[us[0]], None)
                spk = self.engine.ecapa(mel.transpose(1, 2), overlap=True)
                cond = self.gpt.get_conditioning(mel)
                flat = [(u, k, s) for u in us for k, s in enumerate(utt_sents[u])]
                if not flat:
                    continue
                order = sorted(range(len(flat)), key=lambda i: (len(flat[i][2]), i))  # length-sorted decode batches
                rows = self._generate_rows(cond, [flat[i][2] for i in order], g)
                code_rows = [None] * len(flat)
                for i, r in zip(order, rows):
                    code_rows[i] = r
                lats = self._clean_and_latents(cond, [f[2] for f in flat], code_rows, g["max_mel_tokens"],
                                               packed=infer_core.env_switch("ITTS_PACKED_LATENT", self.packed_latent))
                wav_parts = {u: [] for u in us}
                ragged = {"1": True, "0": False}.get(os.environ.get("ITTS_RAGGED_VOCODER", ""), self.ragged_vocoder)
                # equal lengths share a launch sequence; with ragged, unequal ones too; packed: all of them back to back in one item
                if infer_core.env_switch("ITTS_PACKED_VOCODER", self.packed_vocoder):
                    wavs = self.engine.bigvgan_packed(lats, spk)
                else:
                    wavs = self.engine.bigvgan_grouped(lats, spk, ragged=ragged)
                for (u, k, _), wav in zip(flat, wavs):
                    wav_parts[u].append(self._to_int16_range(wav))
                for u in us:
                    if wav_parts[u]:
                        results[u] = wav_parts[u]
        out = []
        for u in range(n):
            if results[u] is None:
                raise RuntimeError(f"IndexTTS.infer_batch: utterance {u} produced no sentences (empty input)")
            out.append(self._finish(results[u], output_paths[u] if output_paths else None, start, (0, 0, 0), False, "batch "))
        return out

    def _infer_batch_mixed(self, prompts, utt_sents, settings, results, admit=False):
        """infer_batch with mixed_batch on: utterances share decode batches whatever their voice, and - with one beam and no
        typical filter - whatever their sampling settings (infer_core.mixed_groups).  Conditioning and the speaker encoder run
        once per distinct prompt object; a decode row carries its prompt's conditioning latents (per-row cond of the prefill) and
        its utterance's entry of the per-row table (Engine.generate with sequences); the latent pass reads its voice through
        cond_index, the vocoder takes one speaker embedding per sentence.  A row's codes, latent and waveform are those of a
        call in which every utterance carries that row's prompt and settings.  results[u] <- the int16-range wave parts.
        admit: a per-row group with more sentences than max_batch (> 6) is ONE generation of max_batch rows whose finished rows
        are refilled from the waiting sentences (Engine.generate(slots=..)) instead of max_batch-sized generations."""
        voice, conds, spks = {}, [], []  # id(prompt) -> index; conditioning [1, latents, D] and speaker embedding [1, E] per voice
        for p in prompts:
            if id(p) not in voice:
                voice[id(p)] = len(conds)
                mel = self._prompt(p, None)
                spks.append(self.engine.ecapa(mel.transpose(1, 2)))
                conds.append(self.gpt.get_conditioning(mel))
        nl, D = self.engine.ccfg.cond_latents, self.engine.ccfg.model_dim
        cond_all = torch.cat([c.reshape(1, nl, D).float() for c in conds], 0)  # [voices, latents, D]
        spk_all = torch.cat([s.reshape(1, -1) for s in spks], 0)
        ragged = {"1": True, "0": False}.get(os.environ.get("ITTS_RAGGED_VOCODER", ""), self.ragged_vocoder)
        for us in infer_core.mixed_groups(settings):
            flat = [(u, k, s) for u in us for k, s in enumerate(utt_sents[u])]
            if not flat:
                continue
            g0 = settings[us[0]]
            kws = {}  # Engine.generate keywords of every utterance of the group (its seed drawn here, in utterance order)
            for u in us:
                g = settings[u]
                kw = infer_core.sampling_kwargs(g["do_sample"], g["num_beams"], g["top_k"], g["top_p"], g["temperature"],
                                                g["typical_sampling"], g["typical_mass"], g["length_penalty"])
                if g.get("seed") is not None:
                    kw["seed"] = int(g["seed"])
                kws[u] = kw
            shared = {k: v for k, v in kws[us[0]].items() if k in ("num_beams", "typical_mass", "length_penalty")}
            per_row = shared.get("num_beams", 1) == 1 and not shared.get("typical_mass")
            order = sorted(range(len(flat)), key=lambda i: (len(flat[i][2]), i))  # length-sorted decode batches
            cap = max(1, self.engine.ccfg.max_batch // max(1, shared.get("num_beams", 1)))
            code_rows = [None] * len(flat)
            one = admit and per_row and cap > 6 and len(order) > cap  # row admission: the whole group in one generation of cap rows
            if one and (self.wide_sampler or os.environ.get("ITTS_WIDE_SAMPLER") or "host") != "device":
                # one whole-vocabulary setting for every row is the scalar request, which takes the host-side token choice here:
                # that path cannot admit rows, so such a group keeps its cap-sized generations
                ents = {infer_core.row_sampling_table(1, kws[u].get("do_sample", False), kws[u].get("top_k", 0), kws[u].get("top_p", 1.0),
                                                      kws[u].get("temperature", 1.0), settings[u]["repetition_penalty"])[0] for u in us}
                e0 = next(iter(ents))
                one = not (len(ents) == 1 and e0[0] == 1 and not 1 <= e0[1] <= 128)
            # admission under beams (admit_beams, on top of admit_rows): a beam group - several beams, no typical filter; mixed_groups
            # made its settings equal - with more sentences than its cap is ONE generation of cap item slots
            nbeam = shared.get("num_beams", 1)
            beam_one = (admit and infer_core.env_switch("ITTS_ADMIT_BEAMS", self.admit_beams) and nbeam > 1
                        and not shared.get("typical_mass") and cap * nbeam > 6 and len(order) > cap)
            if beam_one and kws[us[0]].get("do_sample") and not 1 <= int(kws[us[0]].get("top_k") or 0) <= 128:
                # the whole-vocabulary warpers run on the host unless the device beam sampler was chosen: that path cannot admit
                beam_one = (self.wide_beam_sampler or os.environ.get("ITTS_WIDE_BEAM_SAMPLER") or "host") == "device"
            one = one or beam_one
            for lo in range(0, len(order), len(order) if one else cap):
                sel = order if one else order[lo:lo + cap]
                ids = infer_core.pad_tokens_cat([flat[i][2] for i in sel], self.cfg.gpt.stop_text_token)
                vs = [voice[id(prompts[flat[i][0]])] for i in sel]
                cond = cond_all[vs[0]] if len(set(vs)) == 1 else cond_all[vs]  # one voice: the shared-cond prefill, as without the switch
                if per_row:
                    row = lambda name, default: [kws[flat[i][0]].get(name, default) for i in sel]  # noqa: E731
                    # a sentence's draws: its utterance's seed and its own index in the utterance, whoever shares the batch
                    seeds = [(int(kws[flat[i][0]].get("seed", 0)) * 1000003 + flat[i][1]) % (2 ** 63) for i in sel]
                    kw = dict(do_sample=row("do_sample", False), top_k=row("top_k", 0), top_p=row("top_p", 1.0),
                              temperature=row("temperature", 1.0), seed=seeds,
                              repetition_penalty=[settings[flat[i][0]]["repetition_penalty"] for i in sel])
                else:  # beams / typical filtering: the group shares every setting (mixed_groups), the voices still differ per row
                    kw = dict(kws[us[0]], repetition_penalty=g0["repetition_penalty"])
                if one:
                    kw["slots"] = cap
                if beam_one:
                    kw["admit_beams"] = True
                    kw["admit_min"] = 0.25  # an admission prefills num_beams rows per sentence: 1/4 measured best (profiles/admit_beams.txt)
                codes = self.engine.generate(cond, ids, g0["max_mel_tokens"], wide_sampler=self.wide_sampler,
                                             wide_beam_sampler=self.wide_beam_sampler, retire_rows=self.retire_rows, retire_beams=self.retire_beams, **kw)
                for j, i in enumerate(sel):
                    code_rows[i] = codes[j]
            if any(r[-1] != self.stop_mel_token for r in code_rows):
                warnings.warn(f"WARN: generation stopped due to exceeding `max_mel_tokens` ({g0['max_mel_tokens']}). "
                              "Consider reducing `max_text_tokens_per_sentence` or increasing `max_mel_tokens`.", RuntimeWarning)
            clean = []
            for r in code_rows:
                c, m = infer_core.remove_long_silence(np.asarray(r)[None], self.stop_mel_token)
                clean.append(c[0, : int(m[0])])
            # Latent pass and vocoder: one batch per UTTERANCE (its sentences, its voice through cond_index / per-row spk).  A decode
            # row has the same bits whoever shares its batch; these two stages do not - the latent pass left-pads a batch to its
            # longest sequence, which moves the key tiles of the prefill attention, and the vocoder's few-tile GEMMs choose their
            # tiles by the row count - so batches across utterances would make a request's waveform depend, in
            # its last bits, on the requests it happened to be served with (measured on the micro checkpoint: latents 1e-6,
            # 2.5 % of the int16 samples one unit apart).  The decode steps are where the rows pay; these passes run once.
            # With packed_latent the latent pass has no such dependence (Engine.latent_packed: no pad rows, every sentence tiled from
            # its own key 0, no K split, the GEMM family not chosen by the row count), so the whole decode group shares ONE pass;
            # the vocoder stays per utterance - unless packed_vocoder is on: Engine.bigvgan_packed makes the same promise for the
            # waveform (sentences back to back in one item, no K split, families not chosen by the row count, one speaker row per
            # sentence), so the whole decode group, across utterances and voices, shares ONE vocoder pass.
            cap = self.engine.ccfg.max_batch
            packed_voc = infer_core.env_switch("ITTS_PACKED_VOCODER", self.packed_vocoder)
            held = []  # packed vocoder: (utterance, its latents) of the whole group
            group_lats = None
            if infer_core.env_switch("ITTS_PACKED_LATENT", self.packed_latent):
                group_lats = self.engine.latent_packed(cond_all, [f[2] for f in flat], clean,
                                                       cond_index=[voice[id(prompts[f[0]])] for f in flat])
            for u in us:
                idx = [i for i, f in enumerate(flat) if f[0] == u]
                if not idx:
                    continue
                v = [voice[id(prompts[u])]] * len(idx)
                if group_lats is not None:
                    lats = [group_lats[i] for i in idx]
                else:
                    lats = []
                    for lo in range(0, len(idx), cap):
                        sel = idx[lo:lo + cap]
                        lats.extend(self.engine.latent_batch(cond_all, [flat[i][2] for i in sel], [clean[i] for i in sel], cond_index=v[:len(sel)]))
                if packed_voc:
                    held.append((u, lats))
                    continue
                results[u] = [self._to_int16_range(w) for w in self.engine.bigvgan_grouped(lats, spk_all[v], ragged=ragged)]
            if held:
                rows = [voice[id(prompts[u])] for u, lats in held for _ in lats]
                wavs = self.engine.bigvgan_packed([l for _, lats in held for l in lats], spk_all[rows])
                for u, lats in held:
                    results[u] = [self._to_int16_range(w) for w in wavs[:len(lats)]]
                    wavs = wavs[len(lats):]

    def _prompt(self, prompt_mel, audio_prompt):
        if prompt_mel is None and audio_prompt is None:
            raise TypeError("infer() needs prompt_mel=<tensor> or audio_prompt=<wav path>")
        if prompt_mel is None:
            prompt_mel = self.extract_features(audio_prompt)
        if isinstance(prompt_mel, str):
            prompt_mel = self.extract_features(prompt_mel)
        return prompt_mel.to(self.device)

    def infer(self, prompt_mel=None, text=None, output_path=None, max_text_tokens_per_sentence=120, verbose=False,
              audio_prompt=None, **generation_kwargs):
        return self._synthesize(self._prompt(prompt_mel, audio_prompt), text, output_path, max_text_tokens_per_sentence,
                                10 ** 9, verbose, generation_kwargs, fast=False)

    def infer_stream(self, prompt_mel=None, text=None, audio_prompt=None, chunk_frames=None, first_chunk_frames=None,
                     max_text_tokens_per_sentence=120, check_every=16, **generation_kwargs):
        """`infer` as a generator of (24000, int16 [n, 1]) chunks (not in the reference; opt-in).  The sentences run
        one after another, each on one decode row (at batch 1 the decode step stays on the persistent engine).  Within a sentence
        the codes are fetched every `check_every` decode steps (Engine.generate_stream), cleaned by the causal silence rule
        (infer_core.stream_clean), turned into latent rows by the incremental packed latent pass (Engine.latent_stream) and
        vocoded window by window (Engine.bigvgan_stream): frames [a, b) are emitted as soon as b + R latent rows exist, R =
        Engine.vocoder_reach() - once `first_chunk_frames` frames are final for the sentence's first chunk, `chunk_frames` for the
        later ones; a sentence's end flushes the rest.  Decode steps, latent appends and vocoder windows alternate on the engine's one
        stream; the speaker encoder is joined before the first decode step.  Every chunk is final: the concatenation is, sample for
        sample, the per-sentence composition generate -> stream_clean -> latent_packed -> bigvgan_packed (`infer_batch` on an
        object with packed_latent + packed_vocoder, where stream_clean and remove_long_silence agree - see stream_clean).
        chunk_frames: None = the object's default - ITTS_STREAM_CHUNK, else IndexTTS(stream_chunk_frames=..), else infer_core.STREAM_CHUNK_FRAMES;
        first_chunk_frames: None = min(infer_core.STREAM_FIRST_CHUNK_FRAMES, chunk_frames).  generation kwargs as `infer`, with
        num_beams defaulting to 1 - beams are refused (ValueError, at the call): a beam's prefix is not final - plus `seed`
        (sentence k draws from seed + k; None: drawn from torch's global RNG as `infer` does)."""
        kw = dict(generation_kwargs)
        kw.setdefault("num_beams", 1)
        seed = kw.pop("seed", None)
        g = self._gen_kwargs(kw)
        if g["num_beams"] is not None and int(g["num_beams"]) > 1:
            raise ValueError("infer_stream: num_beams > 1 cannot stream (a beam's prefix is not final); use infer / infer_batch")
        wide = self.wide_sampler or os.environ.get("ITTS_WIDE_SAMPLER") or "host"
        if g["do_sample"] and not 1 <= int(g["top_k"] or 0) <= 128 and wide != "device":
            raise ValueError("infer_stream: top_k outside 1 .. 128 takes the host-side token choice, which cannot stream "
                             "(IndexTTS(wide_sampler='device') runs it on the device)")
        if chunk_frames is None:  # the object's default, which the environment overrides
            chunk_frames = os.environ.get("ITTS_STREAM_CHUNK") or self.stream_chunk_frames or infer_core.STREAM_CHUNK_FRAMES
        chunk = max(1, int(chunk_frames))
        first = max(1, int(first_chunk_frames)) if first_chunk_frames is not None else min(infer_core.STREAM_FIRST_CHUNK_FRAMES, chunk)
        mel = self._prompt(prompt_mel, audio_prompt)
        sents = self._sentences_to_ids(text, max_text_tokens_per_sentence)
        if not sents:
            raise RuntimeError("IndexTTS: the text produced no sentences (empty input)")
        return self._infer_stream(mel, sents, g, seed, chunk, first, int(check_every), wide)

    @torch.no_grad()
    def _infer_stream(self, mel, sents, g, seed, chunk, first, check_every, wide):
        def pcm(wav):
            return self._to_int16_range(wav).type(torch.int16).numpy().T  # what _finish does with a whole utterance

        with self.engine.lock:
            spk = self.engine.ecapa(mel.transpose(1, 2), overlap=True)
            cond = self.gpt.get_conditioning(mel)
            for k, sent in enumerate(sents):
                sample_kw = infer_core.sampling_kwargs(g["do_sample"], 1, g["top_k"], g["top_p"], g["temperature"], g["typical_sampling"],
                                                       g["typical_mass"], g["length_penalty"])
                if seed is not None and "seed" in sample_kw:
                    sample_kw["seed"] = int(seed) + k
                for name in ("num_beams", "length_penalty"):
                    sample_kw.pop(name, None)
                ids = infer_core.pad_tokens_cat([sent], self.cfg.gpt.stop_text_token)
                voc = self.engine.bigvgan_stream(spk, chunk, first)
                state, last_code = None, None
                with self.engine.latent_stream(cond, [sent], g["max_mel_tokens"]) as ls:
                    for new in self.engine.generate_stream(cond, ids, g["max_mel_tokens"], repetition_penalty=g["repetition_penalty"],
                                                           check_every=check_every, wide_sampler=wide, **sample_kw):
                        last_code = int(new[-1])
                        kept, state = infer_core.stream_clean(new, self.stop_mel_token, state=state)
                        if not len(kept):
                            continue
                        wav = voc.push(ls.append([kept])[0])
                        if wav.shape[-1]:
                            yield (24000, pcm(wav))
                if last_code != self.stop_mel_token:
                    warnings.warn(f"WARN: generation stopped due to exceeding `max_mel_tokens` ({g['max_mel_tokens']}). "
                                  "Consider reducing `max_text_tokens_per_sentence` or increasing `max_mel_tokens`.", RuntimeWarning)
                wav = voc.push(None, last=True)
                if wav.shape[-1]:
                    yield (24000, pcm(wav))

    def infer_fast(self, prompt_mel=None, text=None, output_path=None, max_text_tokens_per_sentence=120, verbose=False,
                   sentences_bucket_max_size=4, audio_prompt=None, **generation_kwargs):
        return self._synthesize(self._prompt(prompt_mel, audio_prompt), text, output_path, max_text_tokens_per_sentence,
                                sentences_bucket_max_size, verbose, generation_kwargs, fast=True)
