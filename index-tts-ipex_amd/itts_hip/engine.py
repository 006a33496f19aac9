"""Python face of the HIP engine: owns the weight arena (one contiguous device buffer, so a single RCCL
broadcast replicates a model across ranks), binds it into libitts_hip and exposes the hot-path stages
as tensor-in / tensor-out calls.  torch is used for device memory and streams only."""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import lib as L
from .config import ecapa_dims, perceiver_inner

_TORCH_DT = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.FP8: torch.uint8}
_DT_BYTES = {L.F32: 4, L.BF16: 2, L.FP8: 1}


def make_config(cfg, dtype: int, max_batch: int = 64) -> L.Config:
    g, h, v = cfg["gpt"], cfg["bigvgan"], cfg["vqvae"]
    cm = g["condition_module"]
    c = L.Config()
    c.dtype = dtype
    c.model_dim, c.layers, c.heads = g["model_dim"], g["layers"], g["heads"]
    c.max_mel_tokens, c.max_text_tokens = g["max_mel_tokens"], g["max_text_tokens"]
    c.number_text_tokens, c.number_mel_codes = g["number_text_tokens"], g["number_mel_codes"]
    c.start_mel_token, c.stop_mel_token = g["start_mel_token"], g["stop_mel_token"]
    c.start_text_token, c.stop_text_token = g["start_text_token"], g["stop_text_token"]
    c.cond_latents = g.get("condition_num_latent", 32)
    c.cond_dim, c.cond_ff, c.cond_heads = cm["output_size"], cm["linear_units"], cm["attention_heads"]
    c.cond_blocks, c.cond_idim = cm["num_blocks"], 100
    c.perc_inner, c.perc_layers = perceiver_inner(g), 2
    c.bv_gpt_dim, c.bv_init_ch = h["gpt_dim"], h["upsample_initial_channel"]
    c.bv_num_up = len(h["upsample_rates"])
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        c.bv_up_rates[i], c.bv_up_kernels[i] = u, k
    c.bv_num_res = len(h["resblock_kernel_sizes"])
    c.bv_num_dil = len(h["resblock_dilation_sizes"][0])
    for j, (k, ds) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
        c.bv_res_kernels[j] = k
        for l, d in enumerate(ds):
            c.bv_res_dils[j][l] = d
    c.bv_spk_dim, c.bv_num_mels = h["speaker_embedding_dim"], h["num_mels"]
    e = ecapa_dims(h)
    for i in range(5):
        c.ec_channels[i], c.ec_kernels[i], c.ec_dils[i] = e["channels"][i], e["kernel_sizes"][i], e["dilations"][i]
    c.ec_att, c.ec_scale, c.ec_se = e["attention_channels"], e["res2net_scale"], e["se_channels"]
    c.dv_channels, c.dv_tokens, c.dv_hidden = v["channels"], v["num_tokens"], v["hidden_dim"]
    c.dv_resblocks, c.dv_codebook, c.dv_layers, c.dv_kernel = v["num_resnet_blocks"], v["codebook_dim"], v["num_layers"], v["kernel_size"]
    c.max_batch = max_batch
    return c


class WeightArena:
    """All packed tensors in ONE device buffer (256-byte aligned slots) + a manifest."""

    def __init__(self, packed: Dict[str, Tuple[str, np.ndarray]], dtype: int, device, half=torch.bfloat16):
        """half: the torch dtype of the engine's 16-bit storage type (bfloat16, or float16 for the f16 build of the library)."""
        self.dtype = dtype
        self.half = half
        self.manifest: List[Tuple[str, int, int, Tuple[int, ...]]] = []  # name, offset, dt, shape
        off = 0
        for name, (tag, arr) in packed.items():
            dt = dtype if tag == "w" else (L.FP8 if tag == "q" else L.F32)  # "q": fp8 e4m3 bytes (uint8 array)
            nbytes = int(np.prod(arr.shape)) * _DT_BYTES[dt]
            self.manifest.append((name, off, dt, tuple(int(x) for x in arr.shape)))
            off = (off + nbytes + 255) // 256 * 256
        self.nbytes = off
        self.buf = torch.empty(off, dtype=torch.uint8, device=device)
        # stage through pinned-free host tensors in chunks (bf16 rounding = torch RNE, same as the device cast)
        for (name, o, dt, shape), (tag, arr) in zip(self.manifest, packed.values()):
            if dt == L.FP8:
                t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint8))
                self.buf[o:o + t.numel()].copy_(t.reshape(-1), non_blocking=False)
                continue
            t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
            if dt == L.BF16:
                t = t.to(half)
            n = t.numel() * t.element_size()
            self.buf[o:o + n].copy_(t.reshape(-1).view(torch.uint8), non_blocking=False)

    def view(self, name: str) -> torch.Tensor:
        for n, o, dt, shape in self.manifest:
            if n == name:
                nb = int(np.prod(shape)) * _DT_BYTES[dt]
                return self.buf[o:o + nb].view(self.half if dt == L.BF16 else _TORCH_DT[dt]).view(*shape)
        raise KeyError(name)


class Engine:
    def __init__(self, cfg, dtype: str = "bf16", device: str = "cuda:0", max_batch: int = 64):
        if not torch.cuda.is_available():
            raise RuntimeError("itts_hip.Engine needs an MI355X (no CPU fallback in the product path)")
        # "f16": IEEE half storage (the reference's GPU precision, infer.py:39,44,52) = the second build of the library, in
        # which the 16-bit dtype code means binary16; everything else is the same engine
        self.half_name = "f16" if dtype in ("f16", "fp16", "half") else "bf16"
        self.lib = L.load(self.half_name)
        self.cfg = cfg
        self.dt = {"fp32": L.F32, "f32": L.F32, "bf16": L.BF16, "f16": L.BF16, "fp16": L.BF16, "half": L.BF16}[dtype]
        self.half_dtype = torch.float16 if self.half_name == "f16" else torch.bfloat16
        self.tdt = self.half_dtype if self.dt == L.BF16 else _TORCH_DT[self.dt]
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.side = torch.cuda.Stream(device=self.device)  # ecapa(overlap=True): the speaker encoder beside conditioning / prefill
        self._side_busy = False
        self.ccfg = make_config(cfg, self.dt, max_batch)
        h = C.c_void_p()
        self._ck(self.lib.itts_engine_create(C.byref(self.ccfg), C.byref(h)), "engine_create")
        self.h = h
        self.arenas: List[WeightArena] = []
        # one engine = one decode state + captured graphs: callers on several host threads (the reference web UI starts a
        # worker thread per request into one IndexTTS, webui.py:441-452) serialise on this lock in the drop-in classes
        self.lock = threading.RLock()
        self.up_total = int(np.prod(cfg["bigvgan"]["upsample_rates"]))

    def _ck(self, status, what=""):
        L.check(status, what, self.lib)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                torch.cuda.synchronize(self.device)
                self.lib.itts_engine_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- weights ----
    def load_packed(self, packed: Dict[str, Tuple[str, np.ndarray]], arena: Optional[WeightArena] = None):
        a = arena or WeightArena(packed, self.dt, self.device, self.half_dtype)
        self.arenas.append(a)
        base = a.buf.data_ptr()
        for name, off, dt, shape in a.manifest:
            dims = (C.c_int64 * len(shape))(*shape)
            self._ck(self.lib.itts_engine_bind_tensor(self.h, name.encode(), C.c_void_p(base + off), dt, len(shape), dims),
                    f"bind {name}")
        return a

    def finalize(self):
        self._ck(self.lib.itts_engine_finalize(self.h), "finalize")

    def debug(self, taps: bool = False, force_simple: bool = False, no_graph: bool = False, fuse: bool = False,
              no_engine: bool = False, engine: bool = False):
        """no_engine: keep the five-launches-per-layer decode step instead of the persistent decode engine; engine: use
        the persistent engine (where it applies) whatever ITTS_ENGINE / the built-in default says (A/B, parity tests)."""
        self._ck(self.lib.itts_debug_enable(self.h, int(taps) | (int(force_simple) << 1) | (int(no_graph) << 2) | (int(fuse) << 3)
                                           | (int(no_engine) << 4) | (int(engine) << 5)))

    def fetch_tap(self, name: str) -> np.ndarray:
        n = self.lib.itts_debug_fetch(self.h, name.encode(), None, 0)
        if n < 0:
            raise KeyError(name)
        out = np.empty(n, dtype=np.float32)
        self.lib.itts_debug_fetch(self.h, name.encode(), out.ctypes.data_as(C.c_void_p), n)
        return out

    # ---- helpers ----
    def _s(self):
        return C.c_void_p(self.stream.cuda_stream)

    def _enter(self):
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def _exit(self):
        # (NOT the side stream: the caller's stream is what the next engine call waits for in _enter(), and an overlapped ecapa()
        #  must not hold that call up - its result is joined where it is consumed: _join_side())
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def join_side(self):
        """After ecapa(overlap=True): make the engine's stream AND the caller's current stream wait for the speaker embedding."""
        if self._side_busy:
            torch.cuda.current_stream(self.device).wait_stream(self.side)
        self._join_side()

    def _join_side(self):
        """The engine's own stream waits for an overlapped ecapa(): in front of the decode steps (the persistent decode engine wants
        every CU of the device) and of the vocoder (which reads the embedding)."""
        if self._side_busy:
            self.stream.wait_stream(self.side)
            self._side_busy = False

    def to_act(self, x: torch.Tensor) -> torch.Tensor:
        return x.to(device=self.device, dtype=self.tdt).contiguous()

    # ---- stages ----
    def conditioning(self, mel_bcf: torch.Tensor, length: Optional[int] = None) -> torch.Tensor:
        """mel [1, n_mels, F] (the reference's layout) -> cond fp32 [1, latents, D]; length < F: the prompt is the first
        `length` frames of a padded tensor (get_conditioning with cond_mel_lengths)."""
        assert mel_bcf.ndim == 3 and mel_bcf.shape[0] == 1
        mel = self.to_act(mel_bcf.transpose(1, 2))
        F = mel.shape[1]
        out = torch.empty(1, self.ccfg.cond_latents, self.ccfg.model_dim, dtype=torch.float32, device=self.device)
        self._enter()
        if length is not None and int(length) < F:
            self._ck(self.lib.itts_conditioning_padded(self.h, mel.data_ptr(), int(length), F, out.data_ptr(), self._s()), "conditioning")
        else:
            self._ck(self.lib.itts_conditioning(self.h, mel.data_ptr(), F, out.data_ptr(), self._s()), "conditioning")
        self._exit()
        mel.record_stream(self.stream)
        return out

    def ecapa(self, mel_bfc: torch.Tensor, overlap: bool = False) -> torch.Tensor:
        """mel_ref [B, F, n_mels] -> spk fp32 [B, E].
        overlap=True: enqueued on the engine's SIDE stream (its own scratch arena in the library), so that the engine calls that
        FOLLOW - conditioning, prefill: chains of small kernels, as this one - run beside it (conditioning + speaker encoder 3.65 ->
        2.40 ms at IndexTTS-1.5 sizes).  CONTRACT: the returned tensor is for THIS engine's vocoder calls (bigvgan / bigvgan_grouped
        join the side stream themselves, and so does prefill() in front of the decode steps); any other consumer calls
        join_side() first.  IndexTTS.infer / infer_batch and bench.py use it exactly so."""
        mel = self.to_act(mel_bfc)
        B, F, _ = mel.shape
        out = torch.empty(B, self.ccfg.bv_spk_dim, dtype=torch.float32, device=self.device)
        if overlap:
            self._join_side()  # one overlapped call at a time (one side arena)
            self.side.wait_stream(torch.cuda.current_stream(self.device))
            self._ck(self.lib.itts_ecapa(self.h, mel.data_ptr(), B, F, out.data_ptr(), C.c_void_p(self.side.cuda_stream)), "ecapa")
            self._side_busy = True
            mel.record_stream(self.side)
            out.record_stream(self.side)
            return out
        self._enter()
        self._ck(self.lib.itts_ecapa(self.h, mel.data_ptr(), B, F, out.data_ptr(), self._s()), "ecapa")
        self._exit()
        mel.record_stream(self.stream)
        return out

    def prefill(self, cond: torch.Tensor, text_ids: np.ndarray, max_gen: int, repetition_penalty: float = 10.0,
                suppress_stop: bool = False):
        ids = np.ascontiguousarray(text_ids, dtype=np.int32)
        assert ids.ndim == 2
        B, Lt = ids.shape
        cond = cond.to(device=self.device, dtype=torch.float32).contiguous().view(-1, self.ccfg.model_dim)
        per_row = cond.shape[0] == B * self.ccfg.cond_latents and B > 1  # one prompt per row (a batch of prompts)
        assert per_row or cond.shape[0] == self.ccfg.cond_latents, cond.shape
        self._ck(self.lib.itts_gpt_set_cond_per_row(self.h, int(per_row)), "gpt_set_cond_per_row")
        self._enter()
        self._ck(self.lib.itts_gpt_prefill(self.h, cond.data_ptr(), ids.ctypes.data_as(C.c_void_p), B, Lt, max_gen,
                                          float(repetition_penalty), int(suppress_stop), self._s()), "gpt_prefill")
        self._join_side()  # an overlapped ecapa() ends before the first decode step
        self._gen = (B, max_gen)

    def set_sampling(self, do_sample: bool, top_k: int = 30, top_p: float = 0.8, temperature: float = 1.0,
                     uniforms: Optional[np.ndarray] = None):
        """HF GenerationMixin.sample configuration (infer.py:116-124) for the following prefill/decode calls;
        uniforms [max_gen, B] float32 in [0, 1) are the draws (step k, row b)."""
        if not do_sample:
            self._ck(self.lib.itts_gpt_set_sampling(self.h, 0, 0, 1.0, 1.0, None, 0), "gpt_set_sampling")
            return
        u = np.ascontiguousarray(uniforms, dtype=np.float32)
        self._ck(self.lib.itts_gpt_set_sampling(self.h, 1, int(top_k), float(top_p), float(temperature),
                                               u.ctypes.data_as(C.c_void_p), u.size), "gpt_set_sampling")

    def set_sampling_rows(self, table, uniforms: Optional[np.ndarray] = None):
        """Mixed batch: one (mode, top_k, top_p, temperature, penalty) entry per row for the following single-beam generations
        (itts_gpt_set_sampling_rows; infer_core.row_sampling_table builds the table); uniforms [max_gen, B] are needed when any
        row samples.  Every row's penalty replaces prefill's repetition_penalty.  A table whose rows are all equal is the scalar
        setting (set_sampling) with those values.  None / empty clears the table."""
        if not table:
            self._ck(self.lib.itts_gpt_set_sampling_rows(self.h, None, 0, None, 0), "gpt_set_sampling_rows")
            return
        tab = (L.RowSampling * len(table))(*[L.RowSampling(int(m), int(k), float(p), float(t), float(pen)) for m, k, p, t, pen in table])
        u = None if uniforms is None else np.ascontiguousarray(uniforms, dtype=np.float32)
        self._ck(self.lib.itts_gpt_set_sampling_rows(self.h, tab, len(table), None if u is None else u.ctypes.data_as(C.c_void_p),
                                                    0 if u is None else u.size), "gpt_set_sampling_rows")

    def set_beam_sample(self, num_beams: int, top_k: int = 30, top_p: float = 0.8, temperature: float = 1.0,
                        uniforms: Optional[np.ndarray] = None, do_sample: bool = True, length_penalty: float = 0.0,
                        num_return_sequences: int = 1, host: bool = False):
        """HF beam_sample (do_sample: the reference's default generate() mode, infer.py:116-124; uniforms
        [max_gen, B, 2 * num_beams] float32 in [0, 1)) or beam_search (not do_sample: deterministic) for the following
        generations.  num_beams <= 1 switches beams off.  num_return_sequences: the n best hypotheses per row (fetch
        returns [B * n, max_gen], best first)."""
        if num_beams <= 1:
            self._ck(self.lib.itts_gpt_set_beams(self.h, 1, 1, 1, 1.0, 1.0, 0.0, None, 0), "gpt_set_beams")
            self._ck(self.lib.itts_gpt_set_beam_returns(self.h, 1), "gpt_set_beam_returns")
            self._nb, self._nret = 1, 1
            return
        self._ck(self.lib.itts_gpt_set_beam_returns(self.h, int(num_return_sequences)), "gpt_set_beam_returns")
        self._nret = int(num_return_sequences)
        dev_draws = do_sample and not host  # host: the caller warps and draws (any top_k), the library needs no uniforms
        u = np.ascontiguousarray(uniforms, dtype=np.float32) if dev_draws else None
        self._ck(self.lib.itts_gpt_set_beams(self.h, int(num_beams), int(bool(do_sample)), int(top_k), float(top_p), float(temperature),
                                            float(length_penalty), u.ctypes.data_as(C.c_void_p) if dev_draws else None,
                                            u.size if dev_draws else 0), "gpt_set_beams")
        self._nb = int(num_beams)

    def set_forced(self, ids: Optional[np.ndarray]):
        """Forced tokens [B or 1, n] (int, -1 = free) for the first n steps of the following generations; None clears."""
        if ids is None or np.asarray(ids).size == 0:
            self._ck(self.lib.itts_gpt_set_forced(self.h, None, 0, 0), "gpt_set_forced")
            self._forced = None
            return
        a = np.ascontiguousarray(np.atleast_2d(ids), dtype=np.int32)
        self._ck(self.lib.itts_gpt_set_forced(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1]), "gpt_set_forced")
        self._forced = a  # (generate(slots=) hands every request its own rows of it)

    def set_input_tokens(self, ids: Optional[np.ndarray]):
        """HF `input_tokens` [B or 1, n] (inference_speech, model.py:672-686) for the following generations: forced like
        set_forced, at the reference's positions (token k at mel position k + 1); None clears."""
        if ids is None or np.asarray(ids).size == 0:
            self._ck(self.lib.itts_gpt_set_input_tokens(self.h, None, 0, 0), "gpt_set_input_tokens")
            self._forced = None
            return
        self._forced = None  # (the library's forced table now holds input tokens: nothing for generate(slots=) to hand out)
        a = np.ascontiguousarray(np.atleast_2d(ids), dtype=np.int32)
        self._ck(self.lib.itts_gpt_set_input_tokens(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1]), "gpt_set_input_tokens")

    def decode_mode(self) -> int:
        """1 if the last decode step ran on the persistent decode engine, 0 for the five-launches-per-block path."""
        return int(self.lib.itts_gpt_decode_mode(self.h))

    def set_engine_fp8(self, on: bool = True):
        """Opt-in: a model whose GPT projections and mel_head all carry fp8 copies (build_engine(gpt_fp8="fp8")) runs its 1 - 6 row
        decode steps on the persistent decode engine, streaming the fp8 bytes; off (the default) it keeps the launch path.
        Same codes and logits either way.  ITTS_ENGINE_FP8=0 / 1 in the environment overrides this setting."""
        self._ck(self.lib.itts_gpt_set_engine_fp8(self.h, int(bool(on))), "gpt_set_engine_fp8")

    def set_kv_fp8(self, on: bool = True):
        """Opt-in: the K/V cache of the GPT decode steps as fp8-e4m3 bytes (no scale) instead of the engine's 16-bit type - half
        the cache bytes a decode step streams and half the cache allocation.  16-bit engines only (bf16 and IEEE half; an fp32
        engine raises).  Takes effect at the next prefill; the decode steps then keep the launch path (decode_mode() == 0)
        unless set_engine_kv_fp8 opted the engine object in.  ITTS_KV_FP8=0 / 1 in the environment overrides this setting."""
        self._ck(self.lib.itts_gpt_set_kv_fp8(self.h, int(bool(on))), "gpt_set_kv_fp8")

    def set_engine_kv_fp8(self, on: bool = True):
        """Opt-in, on top of set_kv_fp8: a generation with an fp8 K/V cache runs its 1 - 6 row decode steps (beam rows included) on
        the persistent decode engine, whose attention phase reads and appends the e4m3 rows (decode_mode() == 1); off (the
        default) an fp8 cache keeps the launch path at every row count.  No effect without an fp8 cache.  Both 16-bit engines,
        also together with set_engine_fp8.  ITTS_ENGINE_KV_FP8=0 / 1 in the environment overrides this setting."""
        self._ck(self.lib.itts_gpt_set_engine_kv_fp8(self.h, int(bool(on))), "gpt_set_engine_kv_fp8")

    def decode(self, nsteps: int):
        self._ck(self.lib.itts_gpt_decode(self.h, nsteps, self._s()), "gpt_decode")

    def status(self) -> Tuple[int, int]:
        a, b = C.c_int(), C.c_int()
        self._ck(self.lib.itts_gpt_status(self.h, C.byref(a), C.byref(b), self._s()), "gpt_status")
        return a.value, b.value

    def retire_rows(self) -> int:
        """Opt-in: compact the running generation to its unfinished rows (itts_gpt_retire_rows; synchronises).  The following
        decode steps run at the smaller row count, which is returned; status() counts the live rows, fetch() still returns every
        original row in its original order (retired rows: their codes followed by stop, the logits of their last step before the
        retirement).  A no-op that returns the unchanged count under beams (unless set_retire_beams opted in), host sampling, on
        the persistent engine (<= 6 rows) and when no row or every row has finished."""
        n = C.c_int()
        self._ck(self.lib.itts_gpt_retire_rows(self.h, C.byref(n), self._s()), "gpt_retire_rows")
        return n.value

    def set_retire_beams(self, on: bool = True):
        """Opt-in: retire_rows() also works under beams - it retires the finished batch items of a beam generation, num_beams rows
        as a unit (itts_gpt_set_retire_beams).  A retired item's hypotheses are final and kept by original item: fetch() returns
        [items * num_return_sequences] code rows in the original order, and the bits of the unretired run while the row count
        stays inside one projection-kernel family.  Still a no-op on the persistent engine (<= 6 rows), under host-side beam
        warpers, with `input_tokens`, and when no item or every item is done.  Sticky, default off.  ITTS_RETIRE_BEAMS=0 / 1 in
        the environment overrides this setting."""
        self._ck(self.lib.itts_gpt_set_retire_beams(self.h, int(bool(on))), "gpt_set_retire_beams")
        self._retire_beams = bool(on)

    def rows(self) -> int:
        """Rows the decode steps of the active generation run at (0: no generation)."""
        return int(self.lib.itts_gpt_rows(self.h))

    def keep_row_table(self, on: bool = True):
        """on: the following prefills keep a per-row table that is uniform as a table generation (itts_gpt_keep_row_table), so
        that it can admit rows of other settings (admit_rows)."""
        self._ck(self.lib.itts_gpt_keep_row_table(self.h, int(bool(on))), "gpt_keep_row_table")

    def row_status(self):
        """Per slot of the running generation: (original row, tokens so far, unfinished) as int32 arrays [rows()]."""
        n = self.rows()
        orig, ln, unf = (np.empty(n, dtype=np.int32) for _ in range(3))
        self._ck(self.lib.itts_gpt_row_status(self.h, orig.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p),
                                             unf.ctypes.data_as(C.c_void_p), self._s()), "gpt_row_status")
        return orig, ln, unf

    def admit_rows(self, cond: torch.Tensor, text_ids: np.ndarray, rows=None, uniforms: Optional[np.ndarray] = None,
                   forced: Optional[np.ndarray] = None) -> np.ndarray:
        """Opt-in: refill finished slots of the running generation with new requests (itts_gpt_admit_rows; synchronises).
        text_ids [n, L] with L the text length the generation was prefilled with (pad a shorter text with stop ids); cond one
        [latents, D] block for all n rows or n of them; rows: one (mode, top_k, top_p, temperature, penalty) entry per new row
        (a table generation; None: the generation's own settings); uniforms [n, max_gen]: the draws of sampled rows; forced
        [n, k] (-1 free): only in a generation that was started with forced tokens.  The new rows become original rows
        B0, B0 + 1, ..: fetch() then returns them behind the earlier ones.  The running rows are not stepped.  -> the slots taken.
        Raises (nothing changed) under beams (unless set_admit_beams opted in: see there), typical filtering, host sampling, at <= 6 rows on the persistent engine, after a
        retirement, and when fewer than n slots are finished (a row at max_gen counts as finished)."""
        ids = np.ascontiguousarray(text_ids, dtype=np.int32)
        assert ids.ndim == 2
        n, Lt = ids.shape
        cond = cond.to(device=self.device, dtype=torch.float32).contiguous().view(-1, self.ccfg.model_dim)
        cond_rows, rem = divmod(cond.shape[0], self.ccfg.cond_latents)
        if rem or cond_rows not in (1, n):
            raise ValueError(f"admit_rows: cond {tuple(cond.shape)} for {n} rows")
        tab = None
        if rows is not None:
            if len(rows) != n:
                raise ValueError(f"admit_rows: {len(rows)} settings for {n} rows")
            tab = (L.RowSampling * n)(*[L.RowSampling(int(m), int(k), float(p), float(t), float(pen)) for m, k, p, t, pen in rows])
        u = None if uniforms is None else np.ascontiguousarray(uniforms, dtype=np.float32)
        nb = getattr(self, "_nb", 1)  # under beams (set_admit_beams): n batch items, the draws of every item's 2 * nb picks per step
        if u is not None and u.shape != ((n, self._gen[1]) if nb <= 1 else (n, self._gen[1], 2 * nb)):
            raise ValueError(f"admit_rows: uniforms {u.shape}, expected {(n, self._gen[1]) if nb <= 1 else (n, self._gen[1], 2 * nb)}")
        f = None if forced is None else np.ascontiguousarray(np.atleast_2d(forced), dtype=np.int32)
        if f is not None and f.shape[0] != n:
            raise ValueError(f"admit_rows: forced tokens {f.shape} for {n} rows")
        slots = np.empty(n, dtype=np.int32)
        self._enter()
        self._ck(self.lib.itts_gpt_admit_rows(self.h, cond.data_ptr(), cond_rows, ids.ctypes.data_as(C.c_void_p), n, Lt, tab,
                                             None if u is None else u.ctypes.data_as(C.c_void_p),
                                             None if f is None else f.ctypes.data_as(C.c_void_p), 0 if f is None else f.shape[1],
                                             slots.ctypes.data_as(C.c_void_p), self._s()), "gpt_admit_rows")
        self._gen = (int(self.lib.itts_gpt_rows_total(self.h)) // max(nb, 1), self._gen[1])  # (fetch counts batch items)
        return slots

    def set_admit_beams(self, on: bool = True):
        """Opt-in: admit_rows() also works under beams (itts_gpt_set_admit_beams) - it then admits whole batch items into a
        running beam generation (beam_sample or beam_search on the device): text_ids [n, L] and cond count items, uniforms is
        [n, max_gen, 2 * num_beams] (beam_sample only), rows and forced must stay None, and the returned slots are ITEM slots.
        An item is finished when it is done or holds max_gen tokens; a leaving item's num_return_sequences hypotheses are final and
        kept by original item, the new items become original items behind the earlier ones: fetch() returns
        [items * num_return_sequences] code rows in that order, row_status() stays per row (item i: rows i * num_beams ..).
        Within one projection-kernel family an admitted item's bits are those of a fresh generation of the admitted items.
        retire_rows() (with set_retire_beams) still works afterwards; admission after a retirement does not.  Still refused:
        typical filtering, host-side beam warpers, `input_tokens`, the persistent engine (<= 6 rows).  Sticky, default off.
        ITTS_ADMIT_BEAMS=0 / 1 in the environment overrides this setting."""
        self._ck(self.lib.itts_gpt_set_admit_beams(self.h, int(bool(on))), "gpt_set_admit_beams")
        self._admit_beams = bool(on)

    def fetch(self, logits: bool = False):
        B, mg = self._gen
        codes = np.empty((B * (getattr(self, "_nret", 1) if getattr(self, "_nb", 1) > 1 else 1), mg), dtype=np.int32)
        lg = np.empty((B * getattr(self, "_nb", 1), self.ccfg.number_mel_codes), dtype=np.float32) if logits else None
        self._ck(self.lib.itts_gpt_fetch(self.h, codes.ctypes.data_as(C.c_void_p),
                                        lg.ctypes.data_as(C.c_void_p) if logits else None, self._s()), "gpt_fetch")
        return (codes, lg) if logits else codes

    def generate(self, cond: torch.Tensor, text_ids: np.ndarray, max_gen: int, repetition_penalty: float = 10.0,
                 suppress_stop: bool = False, check_every: int = 16, do_sample: bool = False, top_k: int = 30,
                 top_p: float = 0.8, temperature: float = 1.0, seed: Optional[int] = None,
                 uniforms: Optional[np.ndarray] = None, num_beams: int = 1, typical_mass: float = 0.0,
                 length_penalty: float = 0.0, num_return_sequences: int = 1, wide_sampler: Optional[str] = None,
                 wide_beam_sampler: Optional[str] = None, retire_rows: Optional[float] = None, slots: Optional[int] = None,
                 admit_min: float = 0.125, return_log: bool = False, retire_beams: Optional[bool] = None,
                 admit_beams: Optional[bool] = None) -> np.ndarray:
        """Greedy decode (do_sample=False, num_beams=1 of tests/padding_test.py:35-46) or, with do_sample, HF
        GenerationMixin.sample (top-k / top-p / temperature, num_beams=1; draws from `uniforms` or a numpy Generator
        seeded with `seed`).  Returns int64 codes [B, n] with n <= max_gen: HF stops when every row has emitted stop
        or at max length.  num_beams > 1: HF beam_sample (do_sample; uniforms [max_gen, B, 2 * num_beams]) or beam_search
        (not do_sample) over num_beams beams per row; returns the best finalized hypothesis per row, or with
        num_return_sequences = n the n best of every row ([B * n, len], best first).
        wide_sampler: how do_sample with one beam and top_k outside 1 .. 128 (0 / None = HF's TopK warper off) runs - "host"
        (the default): the token choice on the host with torch's arithmetic, bit for bit, one stream sync per token; "device":
        sampler_wide_kernel, no sync per token, graph replay - the same distribution with parallel fp32 sums, so the top-p
        boundary and the draw agree with the host's to 64 * 2^-24 of the mass, not to the last bit.  None: the environment's
        ITTS_WIDE_SAMPLER, else "host".  Requests with beams ignore it.
        wide_beam_sampler: the same choice for do_sample with several beams and top_k outside 1 .. 128 - "host" (the default):
        warpers and draws on the host (infer_core.host_beam_step: torch's arithmetic, a logits and beam-state read-back and two
        stream syncs per token); "device": beam_wide_cand_kernel + beam_wide_pick_kernel in front of beam_select_kernel, no
        read-back, graph replay - the same distribution with parallel fp32 sums, top-p boundary and draws within 512 * 2^-24 of
        the mass of the host's.  None: the environment's ITTS_WIDE_BEAM_SAMPLER, else "host".
        retire_rows: opt-in row retirement of a batched single-beam generation - a ratio r in (0, 1]: after a status() the loop
        calls retire_rows() whenever unfinished <= r * rows() and rows() > 6 (at six rows and below the persistent engine is the
        better place to be, and it cannot follow a retirement).  Same codes within one projection-kernel family; across families
        (e.g. 12 -> 3 rows) within the project's cross-family bound.  None: the environment's ITTS_RETIRE_ROWS, else off.
        Suggested value: 0.5 - measured with tools/bench_row_retire.py (profiles/row_retire.txt): 64 ragged
        rows decode 1.18 x faster at 0.5 and 1.19 x at 0.75; 20 rows with fp8 weights gain nothing at 0.5 and lose 3 % at 0.75.
        retire_beams: opt-in on top of retire_rows for num_beams > 1 (set_retire_beams for the duration of the call): the loop
        applies the same rule to a beam generation and retires its finished batch items, num_beams rows as a unit.  Off, a beam
        generation ignores retire_rows as before.  None: the environment's ITTS_RETIRE_BEAMS, else off.  Measured with
        tools/bench_beam_retire.py (profiles/beam_retire.txt).
        Mixed batches: do_sample, top_k, top_p, temperature, repetition_penalty and seed also take a sequence of length B, one
        entry per row (single beam, no typical filter: ValueError otherwise).  Entries that are all equal - with one seed - are the
        scalar request, on today's path.  Otherwise every row chooses its tokens with its own entry (infer_core.row_sampling_table,
        itts_gpt_set_sampling_rows) and gets the codes of a generation of the same rows in which every row carries that entry.
        With per-row seeds column b of the draws is np.random.default_rng(seed[b]).random(max_gen, dtype=float32): a row's draws
        do not depend on who shares its batch.  In a table that is not uniform a row with top_k outside 1 .. 128 always runs on
        the device's whole-vocabulary sampler - the host path cannot mix - whatever wide_sampler says.
        Row admission (opt-in): slots=S with more than S rows in text_ids (and in the per-row sequences; cond shared or one block
        per row) decodes them as ONE generation of S rows - the S longest texts start, and after each status check rows from the
        waiting list take the slots of finished rows (admit_rows) whenever at least ceil(admit_min * S) slots are finished or
        the rest of the list fits; once the list is empty retire_rows applies as above.  The loop ends when the list is empty
        and no row is live (a row at max_gen counts as finished).  Codes come back in the caller's order; return_log=True also
        returns the admissions as (tokens decoded so far, slots, request indices).  Single beam, no typical filter, more than 6
        slots.  Device samplers only: one sampled setting for every request with top_k outside 1 .. 128 needs
        wide_sampler="device" (ValueError otherwise: the host path cannot admit); in a table that is not uniform such rows run
        on the device as above.  Forced tokens given to set_forced for all N requests (or one row for all) follow their requests.
        Suggested admit_min: 0.125, the default - measured with tools/bench_admit_rows.py (profiles/admit_rows.txt, DESIGN.md
        section 5i): 192 ragged requests through 64 slots take 1708 ms at 1/8, 1746 ms at 1/4 and 1932 ms at 1/2 against 2149 ms
        as three 64-row generations (1900 ms with retire_rows=0.5): an admission of 8 rows costs 5 ms, about three token steps, so
        small groups do not lose.
        admit_beams: opt-in on top of slots= for num_beams > 1 (set_admit_beams for the duration of the call): S counts batch
        ITEMS (S * num_beams rows, <= max_batch and > 6), whole items are admitted and leave, uniforms is (max_gen, N, 2 *
        num_beams) by request (drawn from `seed` when absent), num_return_sequences is allowed and the result is [N * returns, n]
        in the caller's order; the log holds item slots.  One setting for all requests, no typical filter; do_sample with top_k
        outside 1 .. 128 needs wide_beam_sampler="device" (ValueError otherwise).  Once the list is empty retire_rows applies only
        together with retire_beams.  Off, slots= with beams raises as before.  None: the environment's ITTS_ADMIT_BEAMS, else off.
        Measured with tools/bench_admit_beams.py (profiles/admit_beams.txt)."""
        rows = None
        per_row = dict(do_sample=do_sample, top_k=top_k, top_p=top_p, temperature=temperature, repetition_penalty=repetition_penalty)
        if any(isinstance(v, (list, tuple, np.ndarray)) for v in list(per_row.values()) + [seed]):
            from . import infer_core

            if num_beams > 1 or typical_mass:
                raise ValueError("per-row sampling settings run with one beam and without typical filtering only")
            nrow = np.asarray(text_ids).shape[0]
            table = infer_core.row_sampling_table(nrow, **per_row)
            seeds = list(seed) if isinstance(seed, (list, tuple, np.ndarray)) else [seed] * nrow
            if len(seeds) != nrow:
                raise ValueError(f"seed has {len(seeds)} entries for {nrow} rows")
            one_seed = all(s == seeds[0] for s in seeds)
            if uniforms is None and not one_seed and any(r[0] for r in table):
                uniforms = infer_core.row_uniforms(seeds, max_gen)
            seed = seeds[0]
            if all(r == table[0] for r in table):  # the scalar request
                mode, top_k, top_p, temperature, repetition_penalty = table[0]
                do_sample = bool(mode)
            else:
                if uniforms is None and any(r[0] for r in table):
                    uniforms = np.random.default_rng(seed).random((max_gen, nrow), dtype=np.float32)
                rows, do_sample, repetition_penalty = table, False, table[0][4]
        if retire_rows is None:
            retire_rows = float(os.environ.get("ITTS_RETIRE_ROWS") or 0.0)
        retire_rows = float(retire_rows)
        if not 0.0 <= retire_rows <= 1.0:
            raise ValueError(f"retire_rows must be a ratio in (0, 1] (or 0 / None: off), not {retire_rows!r}")
        if retire_beams is None:
            retire_beams = bool(int(os.environ.get("ITTS_RETIRE_BEAMS") or 0))
        if wide_sampler is None:
            wide_sampler = os.environ.get("ITTS_WIDE_SAMPLER") or "host"
        if wide_sampler not in ("host", "device"):
            raise ValueError(f"wide_sampler must be 'host' or 'device', not {wide_sampler!r}")
        if wide_beam_sampler is None:
            wide_beam_sampler = os.environ.get("ITTS_WIDE_BEAM_SAMPLER") or "host"
        if wide_beam_sampler not in ("host", "device"):
            raise ValueError(f"wide_beam_sampler must be 'host' or 'device', not {wide_beam_sampler!r}")
        if admit_beams is None:
            admit_beams = bool(int(os.environ.get("ITTS_ADMIT_BEAMS") or 0))
        if slots is not None and np.asarray(text_ids).shape[0] > int(slots) and num_beams > 1 and admit_beams:
            nb, S = int(num_beams), int(slots)
            if typical_mass:
                raise ValueError("row admission under beams (slots=, admit_beams=True) runs without typical filtering only")
            if rows is not None:
                raise ValueError("row admission under beams (slots=, admit_beams=True) takes one setting for every request")
            if do_sample and not 1 <= int(top_k or 0) <= 128 and wide_beam_sampler != "device":
                raise ValueError("row admission under beams (slots=, admit_beams=True) with top_k outside 1 .. 128 runs on the device's "
                                 "whole-vocabulary beam sampler only: pass wide_beam_sampler='device' (the host-side warpers cannot admit)")
            if not 6 < S * nb <= self.ccfg.max_batch:
                raise ValueError(f"row admission under beams: slots * num_beams = {S * nb} must be above 6 (the persistent engine's "
                                 f"rows) and at most max_batch = {self.ccfg.max_batch}")
            nrow = np.asarray(text_ids).shape[0]
            if do_sample and uniforms is None:
                uniforms = np.random.default_rng(seed).random((max_gen, nrow, 2 * nb), dtype=np.float32)
            out = self._generate_admit_beams(cond, text_ids, max_gen, S, float(admit_min), suppress_stop, check_every, retire_rows,
                                             bool(retire_beams), bool(do_sample), int(top_k or 0), top_p, temperature,
                                             uniforms if do_sample else None, nb, length_penalty, int(num_return_sequences),
                                             float(repetition_penalty))
            return out if return_log else out[0]
        if slots is not None and np.asarray(text_ids).shape[0] > int(slots):
            if num_beams > 1 or typical_mass:
                raise ValueError("row admission (slots=) runs with one beam and without typical filtering only")
            nrow = np.asarray(text_ids).shape[0]
            scalar = None
            if rows is None:  # one setting for every request
                scalar = (int(bool(do_sample)), int(top_k or 0) if do_sample else 0, float(top_p), float(temperature), float(repetition_penalty))
                if do_sample and not 1 <= scalar[1] <= 128 and wide_sampler != "device":
                    raise ValueError("row admission (slots=) with top_k outside 1 .. 128 runs on the device's whole-vocabulary sampler "
                                     "only: pass wide_sampler='device' (the host-side token choice cannot admit rows)")
                if do_sample and uniforms is None:
                    uniforms = np.random.default_rng(seed).random((max_gen, nrow), dtype=np.float32)
            out = self._generate_admit(cond, text_ids, max_gen, rows, scalar, uniforms, int(slots), float(admit_min), suppress_stop,
                                       check_every, retire_rows)
            return out if return_log else out[0]
        if return_log:
            raise ValueError("return_log needs slots= and more rows than slots")
        kw = dict(retire_rows=retire_rows, retire_beams=bool(retire_beams), wide_sampler=wide_sampler, wide_beam_sampler=wide_beam_sampler, repetition_penalty=repetition_penalty, suppress_stop=suppress_stop, check_every=check_every, do_sample=do_sample,
                  top_k=top_k, top_p=top_p, temperature=temperature, seed=seed, uniforms=uniforms, num_beams=num_beams,
                  typical_mass=typical_mass, length_penalty=length_penalty, num_return_sequences=num_return_sequences, rows=rows)
        try:
            return self._generate_once(cond, text_ids, max_gen, **kw)
        except L.HandoffTimeout as e:
            # The persistent decode engine needs every CU of its GPU; a wait inside it gave up (another process or a long
            # foreign kernel held CUs).  The library has switched this engine object to the launch path: redo the utterance
            # there, once, in this process - same prefill, same uniforms / seed, so the same ids as an undisturbed run.
            _warn_downgrade(e)
            return self._generate_once(cond, text_ids, max_gen, **kw)

    def _generate_once(self, cond, text_ids, max_gen, repetition_penalty, suppress_stop, check_every, do_sample, top_k, top_p,
                       temperature, seed, uniforms, num_beams, typical_mass, length_penalty, num_return_sequences,
                       wide_sampler="host", wide_beam_sampler="host", retire_rows=0.0, rows=None, retire_beams=False) -> np.ndarray:
        """rows: the per-row table of a mixed batch (generate; do_sample is False then and the scalar settings are not read)."""
        beams = num_beams > 1
        if num_return_sequences != 1 and not beams:
            raise ValueError("num_return_sequences > 1 without beams: repeat the rows (indextts/gpt/model.py does, as HF does)")
        nrow = np.asarray(text_ids).shape[0]
        if do_sample and (not top_k or int(top_k) < 1 or int(top_k) > 128):
            # HF: TopK warper off (top_k = 0 / None) or wider than the narrow device samplers' 128 candidates - exact on the
            # host, or (one beam, wide_sampler="device"; beams, wide_beam_sampler="device") the whole-vocabulary device samplers
            # through the ordinary loop below
            if beams and wide_beam_sampler != "device":
                return self._generate_host_beams(cond, text_ids, max_gen, repetition_penalty, suppress_stop, int(top_k or 0), top_p,
                                                 temperature, seed, uniforms, typical_mass, num_beams, length_penalty,
                                                 num_return_sequences)
            if not beams and wide_sampler != "device":
                return self._generate_host_sampled(cond, text_ids, max_gen, repetition_penalty, suppress_stop, int(top_k or 0),
                                                   top_p, temperature, seed, uniforms, typical_mass)
            top_k = int(top_k or 0)
        typical = bool(typical_mass)
        if typical:  # typical_sampling=True (model.py:690-697): TypicalLogitsWarper behind the repetition penalty, in every mode
            self._ck(self.lib.itts_gpt_set_typical(self.h, float(typical_mass)), "gpt_set_typical")
        if beams:
            if uniforms is None and do_sample:
                uniforms = np.random.default_rng(seed).random((max_gen, nrow, 2 * num_beams), dtype=np.float32)
            self.set_beam_sample(num_beams, top_k, top_p, temperature, uniforms, do_sample=do_sample, length_penalty=length_penalty,
                                 num_return_sequences=num_return_sequences)
        elif do_sample:
            if uniforms is None:
                uniforms = np.random.default_rng(seed).random((max_gen, nrow), dtype=np.float32)
            self.set_sampling(True, top_k, top_p, temperature, uniforms)
        retire_beams = bool(retire_beams and retire_rows and beams)
        held_rb = getattr(self, "_retire_beams", False)  # what set_retire_beams holds: the caller's setting
        try:
            if rows is not None:
                self.set_sampling_rows(rows, uniforms)
            if retire_beams:
                self.set_retire_beams(True)
            self.prefill(cond, text_ids, max_gen, repetition_penalty, suppress_stop)
            done = 1
            while done < max_gen:
                if not suppress_stop:
                    step, unf = self.status()
                    done = step
                    if unf == 0:
                        break
                    if retire_rows and (not beams or retire_beams):
                        rows_now = self.rows()
                        if rows_now > 6 and unf <= retire_rows * rows_now:
                            self.retire_rows()
                n = min(check_every, max_gen - done)
                self.decode(n)
                done += n
            step, unf = self.status()
            codes = self.fetch()[:, :step].astype(np.int64)
            self._exit()
        finally:
            if typical:
                self._ck(self.lib.itts_gpt_set_typical(self.h, 0.0), "gpt_set_typical")
            if beams:
                self.set_beam_sample(1)
            elif do_sample:
                self.set_sampling(False)
            if rows is not None:
                self.set_sampling_rows(None)
            if retire_beams:
                self.set_retire_beams(held_rb)  # the caller's setting, as it was
        # HF stops right after the step in which the last running row emitted stop: trim the look-ahead steps
        stop = self.ccfg.stop_mel_token
        n = 0
        for row in codes:
            hit = np.nonzero(row == stop)[0]
            n = max(n, int(hit[0]) + 1 if len(hit) else step)
        return codes[:, :n]

    def generate_stream(self, cond: torch.Tensor, text_ids: np.ndarray, max_gen: int, repetition_penalty: float = 10.0,
                        check_every: int = 16, do_sample: bool = False, top_k: int = 30, top_p: float = 0.8, temperature: float = 1.0,
                        seed: Optional[int] = None, uniforms: Optional[np.ndarray] = None, num_beams: int = 1,
                        typical_mass: float = 0.0, wide_sampler: Optional[str] = None, input_tokens=None, suppress_stop: bool = False):
        """The _generate_once loop as a GENERATOR, for one row and one beam: after the prefill and after every `check_every`
        decode steps it fetches and yields the codes decoded since the last yield (int64 [n], the stop token included; the
        generation ends behind it or at max_gen).  Greedy, device sampling (top_k 1 .. 128, or any top_k with
        wide_sampler="device"), typical filtering and the repetition penalty; the same prefill, steps and uniforms as
        generate(), so the codes yielded are generate()'s.  Between two yields the engine's stream is free for the caller's
        latent appends and vocoder windows (no decode buffer moves; nothing runs beside a decode step).
        ValueError: num_beams > 1 (a beam's prefix is not final), host-side sampling (top_k outside 1 .. 128 without
        wide_sampler="device"), input_tokens, more than one row.  Checked here, before the generator is returned.
        suppress_stop: the stop token cannot be chosen (bench.py's forced length): the generation runs to max_gen."""
        ids = np.ascontiguousarray(text_ids, dtype=np.int32)
        ids = ids[None] if ids.ndim == 1 else ids
        if ids.shape[0] != 1:
            raise ValueError(f"generate_stream: one row, not {ids.shape[0]}")
        if num_beams is not None and int(num_beams) > 1:
            raise ValueError("generate_stream: num_beams > 1 cannot stream - a beam's prefix is not final until the search ends")
        if input_tokens is not None:
            raise ValueError("generate_stream: input_tokens are not supported")
        if wide_sampler is None:
            wide_sampler = os.environ.get("ITTS_WIDE_SAMPLER") or "host"
        if do_sample and (not top_k or int(top_k) < 1 or int(top_k) > 128) and wide_sampler != "device":
            raise ValueError("generate_stream: top_k outside 1 .. 128 takes the host-side token choice, which cannot stream; pass "
                             "wide_sampler='device' for the whole-vocabulary device sampler")
        max_gen = int(max_gen)
        if do_sample and uniforms is None:
            uniforms = np.random.default_rng(seed).random((max_gen, 1), dtype=np.float32)
        return self._generate_stream(cond, ids, max_gen, float(repetition_penalty), max(1, int(check_every)), bool(do_sample),
                                     int(top_k or 0), top_p, temperature, uniforms, float(typical_mass or 0.0), bool(suppress_stop))

    def _generate_stream(self, cond, ids, max_gen, repetition_penalty, check_every, do_sample, top_k, top_p, temperature, uniforms,
                         typical_mass, suppress_stop=False):
        stop = self.ccfg.stop_mel_token
        sent = 0  # codes yielded so far
        for attempt in (0, 1):
            try:
                if typical_mass:
                    self._ck(self.lib.itts_gpt_set_typical(self.h, typical_mass), "gpt_set_typical")
                if do_sample:
                    self.set_sampling(True, top_k, top_p, temperature, uniforms)
                try:
                    self.prefill(cond, ids, max_gen, repetition_penalty, suppress_stop)
                    while True:
                        step, unf = self.status()
                        row = self.fetch()[0, :step].astype(np.int64)
                        hit = np.nonzero(row == stop)[0]
                        end = int(hit[0]) + 1 if len(hit) else step
                        if end > sent:
                            new, sent = row[sent:end], end
                            yield new
                        if unf == 0 or len(hit) or step >= max_gen:
                            break
                        self.decode(min(check_every, max_gen - step))
                    self._exit()
                finally:
                    if typical_mass:
                        self._ck(self.lib.itts_gpt_set_typical(self.h, 0.0), "gpt_set_typical")
                    if do_sample:
                        self.set_sampling(False)
                return
            except L.HandoffTimeout as e:
                # as generate(): the library has switched this engine object to the launch path; the utterance is decoded again from
                # its prefill with the same draws, and the codes already yielded are skipped
                if attempt:
                    raise
                _warn_downgrade(e)

    def _generate_admit(self, cond, text_ids, max_gen, table, scalar, uniforms, slots, admit_min, suppress_stop, check_every,
                        retire_rows):
        """generate(slots=..): one generation of `slots` rows over all N requests (infer_core.AdmitScheduler says who starts and
        who takes which finished slot).  table: the N per-row entries, or None with `scalar` = the one entry of every request;
        uniforms [max_gen, N] by request (None: nobody draws).  -> (codes int64 [N, n] in the caller's order, the admission log)"""
        from . import infer_core

        ids = np.ascontiguousarray(text_ids, dtype=np.int32)
        N = ids.shape[0]
        cc = self.ccfg
        lengths = [int(np.count_nonzero((r != cc.start_text_token) & (r != cc.stop_text_token))) for r in ids]
        sched = infer_core.AdmitScheduler(lengths, slots, admit_min)
        cond = cond.to(device=self.device, dtype=torch.float32).contiguous().view(-1, cc.cond_latents, cc.model_dim)
        if cond.shape[0] not in (1, N):
            raise ValueError(f"generate(slots=): cond holds {cond.shape[0]} blocks for {N} rows")
        cond_of = (lambda req: cond[0]) if cond.shape[0] == 1 else (lambda req: cond[list(req)])
        u = None if uniforms is None else np.ascontiguousarray(uniforms, dtype=np.float32).reshape(max_gen, N)
        entry = (lambda r: table[r]) if table is not None else (lambda r: scalar)
        log, stop = [], cc.stop_mel_token
        first = sched.first
        held = getattr(self, "_forced", None)  # what set_forced holds: one row for all, or one per request
        if held is not None and held.shape[0] not in (1, N):
            raise ValueError(f"generate(slots=): forced tokens were set for {held.shape[0]} rows, not for 1 or {N}")
        fo = None if held is None else np.ascontiguousarray(np.broadcast_to(held, (N, held.shape[1])))
        try:
            if fo is not None:
                self.set_forced(fo[first])
            if table is not None:
                self.keep_row_table(True)
                self.set_sampling_rows([table[r] for r in first], None if u is None else u[:, first])
            elif scalar[0]:
                self.set_sampling(True, scalar[1], scalar[2], scalar[3], u[:, first])
            self.prefill(cond_of(first), ids[first], max_gen, entry(first[0])[4], suppress_stop)
            steps, retired = 1, False
            while True:
                orig, ln, unf = self.row_status()
                live = (unf != 0) & (ln < max_gen)
                if sched.waiting and not retired:
                    sl, req = sched.take(np.nonzero(~live)[0].tolist())
                    if req:
                        draws = u is not None and any(entry(r)[0] for r in req)
                        took = self.admit_rows(cond_of(req), ids[req], rows=None if table is None else [table[r] for r in req],
                                               uniforms=np.ascontiguousarray(u[:, req].T) if draws else None,
                                               forced=None if fo is None else fo[req])
                        assert took.tolist() == sl, (took, sl)
                        log.append((steps, sl, req))
                        ln[sl], live[sl] = 1, True  # (a forced first stop shows at the next status)
                if not sched.waiting:
                    if not live.any():
                        break
                    rows_now = self.rows()
                    if retire_rows and rows_now > 6 and int(live.sum()) <= retire_rows * rows_now and int(live.sum()) < rows_now:
                        if self.retire_rows() != rows_now:  # the slots are another set now; only the live rows' counts are read below
                            retired = True
                            ln, live = ln[live], live[live]
                n = min(check_every, max_gen - int(ln[live].min())) if live.any() else check_every
                self.decode(n)
                steps += n
            orig, ln, unf = self.row_status()
            codes = self.fetch().astype(np.int64)
            for s, j in enumerate(orig):
                codes[j, ln[s]:] = stop  # behind a row's own tokens the slot holds what an earlier row left
            self._exit()
        finally:
            if fo is not None:
                self.set_forced(held)  # the caller's setting, as it was
            if table is not None:
                self.set_sampling_rows(None)
                self.keep_row_table(False)
            # a table whose FIRST rows are all equal is the scalar setting to the library (it sets do_sample and keeps the draws):
            # nothing of this call may stay behind for the next generation
            self.set_sampling(False)
        order = sched.order()
        assert sorted(order) == list(range(N)) and codes.shape[0] == N, (order, codes.shape)
        out = np.empty_like(codes)
        out[order] = codes
        n = 0
        for row in out:
            hit = np.nonzero(row == stop)[0]
            n = max(n, int(hit[0]) + 1 if len(hit) else max_gen)
        return out[:, :n], log

    def _generate_admit_beams(self, cond, text_ids, max_gen, slots, admit_min, suppress_stop, check_every, retire_rows, retire_beams,
                              do_sample, top_k, top_p, temperature, uniforms, num_beams, length_penalty, num_return_sequences,
                              repetition_penalty):
        """generate(slots=.., num_beams > 1, admit_beams=True): one beam generation of `slots` batch items over all N requests;
        infer_core.AdmitScheduler runs with items as slots.  uniforms [max_gen, N, 2 * num_beams] by request (None: beam_search).
        -> (codes int64 [N * num_return_sequences, n] in the caller's order, the admission log with item slots)"""
        from . import infer_core

        ids = np.ascontiguousarray(text_ids, dtype=np.int32)
        N, nb, nret = ids.shape[0], num_beams, num_return_sequences
        cc = self.ccfg
        lengths = [int(np.count_nonzero((r != cc.start_text_token) & (r != cc.stop_text_token))) for r in ids]
        sched = infer_core.AdmitScheduler(lengths, slots, admit_min)
        cond = cond.to(device=self.device, dtype=torch.float32).contiguous().view(-1, cc.cond_latents, cc.model_dim)
        if cond.shape[0] not in (1, N):
            raise ValueError(f"generate(slots=): cond holds {cond.shape[0]} blocks for {N} rows")
        cond_of = (lambda req: cond[0]) if cond.shape[0] == 1 else (lambda req: cond[list(req)])
        u = None if uniforms is None else np.ascontiguousarray(uniforms, dtype=np.float32).reshape(max_gen, N, 2 * nb)
        log, stop = [], cc.stop_mel_token
        first = sched.first
        retire = bool(retire_rows and retire_beams)
        held_ab, held_rb = getattr(self, "_admit_beams", False), getattr(self, "_retire_beams", False)  # the caller's settings
        try:
            self.set_admit_beams(True)
            if retire:
                self.set_retire_beams(True)
            self.set_beam_sample(nb, top_k, top_p, temperature, None if u is None else u[:, first], do_sample=do_sample,
                                 length_penalty=length_penalty, num_return_sequences=nret)
            self.prefill(cond_of(first), ids[first], max_gen, repetition_penalty, suppress_stop)
            steps, retired = 1, False
            while True:
                orig, ln, unf = self.row_status()
                il, iu = ln[::nb].copy(), unf[::nb]  # per item: an item's rows step together
                live = (iu != 0) & (il < max_gen)
                if sched.waiting and not retired:
                    sl, req = sched.take(np.nonzero(~live)[0].tolist())
                    if req:
                        took = self.admit_rows(cond_of(req), ids[req],
                                               uniforms=None if u is None else np.ascontiguousarray(u[:, req].transpose(1, 0, 2)))
                        assert took.tolist() == sl, (took, sl)
                        log.append((steps, sl, req))
                        il[sl], live[sl] = 1, True
                if not sched.waiting:
                    if not live.any():
                        break
                    rows_now = self.rows()
                    n_live = int(live.sum()) * nb
                    if retire and rows_now > 6 and n_live <= retire_rows * rows_now and n_live < rows_now:
                        if self.retire_rows() != rows_now:  # the item slots are another set now: read them again
                            retired = True
                            continue
                n = min(check_every, max_gen - int(il[live].min())) if live.any() else check_every
                self.decode(n)
                steps += n
            codes = self.fetch().astype(np.int64)  # [N * nret, max_gen] by original item, stop behind every hypothesis
            self._exit()
        finally:
            self.set_beam_sample(1)
            if retire:
                self.set_retire_beams(held_rb)
            self.set_admit_beams(held_ab)
        order = sched.order()
        assert sorted(order) == list(range(N)) and codes.shape[0] == N * nret, (order, codes.shape)
        out = np.empty_like(codes).reshape(N, nret, max_gen)
        out[order] = codes.reshape(N, nret, max_gen)
        out = out.reshape(N * nret, max_gen)
        n = 0
        for row in out:
            hit = np.nonzero(row == stop)[0]
            n = max(n, int(hit[0]) + 1 if len(hit) else max_gen)
        return out[:, :n], log

    def _generate_host_sampled(self, cond, text_ids, max_gen, repetition_penalty, suppress_stop, top_k, top_p, temperature, seed,
                               uniforms, typical_mass) -> np.ndarray:
        """HF sample() with the token choice on the host (infer_core.host_sample_step: warpers over the WHOLE vocabulary): the
        step stops behind the head GEMV, the logits come back, the chosen tokens go in through itts_gpt_commit.  One stream
        sync per token - the price of torch's own arithmetic, bit for bit.  generate(wide_sampler="device") runs the same mode on
        the device (sampler_wide_kernel: no sync per token; parallel fp32 sums, equal to this path within 64 * 2^-24 of the mass)."""
        from . import infer_core

        nrow = np.asarray(text_ids).shape[0]
        if uniforms is None:
            uniforms = np.random.default_rng(seed).random((max_gen, nrow), dtype=np.float32)
        stop, start = self.ccfg.stop_mel_token, self.ccfg.start_mel_token
        seen = [{1, start} for _ in range(nrow)]  # fake prefix ids are all 1, the last one start_mel (model.py:644-653)
        unfinished = np.ones(nrow, dtype=bool)
        out = np.full((nrow, max_gen), stop, dtype=np.int64)
        n = 0
        self._ck(self.lib.itts_gpt_set_host_sampling(self.h, 1), "gpt_set_host_sampling")
        try:
            self.prefill(cond, text_ids, max_gen, repetition_penalty, suppress_stop)
            for k in range(max_gen):
                _, lg = self.fetch(logits=True)
                toks = infer_core.host_sample_step(lg, seen, float(repetition_penalty), float(temperature), top_k, top_p,
                                                   float(typical_mass or 0.0), uniforms[k], stop, bool(suppress_stop))
                toks = np.where(unfinished, toks, stop).astype(np.int32)
                self._ck(self.lib.itts_gpt_commit(self.h, toks.ctypes.data_as(C.c_void_p), self._s()), "gpt_commit")
                out[:, k] = toks
                n = k + 1
                for r in range(nrow):
                    seen[r].add(int(toks[r]))
                unfinished &= toks != stop
                if not unfinished.any() or n == max_gen:
                    break
                self.decode(1)
            self._exit()
        finally:
            self._ck(self.lib.itts_gpt_set_host_sampling(self.h, 0), "gpt_set_host_sampling")
        return out[:, :n]

    def _generate_host_beams(self, cond, text_ids, max_gen, repetition_penalty, suppress_stop, top_k, top_p, temperature, seed,
                             uniforms, typical_mass, num_beams, length_penalty, num_return_sequences) -> np.ndarray:
        """HF beam_sample with the warpers and the draws on the host (infer_core.host_beam_step: any top_k, whole vocabulary),
        BeamSearchScorer.process / beam re-ordering / finalize on the device (itts_gpt_commit_beams).  One logits + beam-state
        read-back per token - the price of torch's own arithmetic, bit for bit.  generate(wide_beam_sampler="device") runs the same
        mode on the device (beam_wide_cand_kernel / beam_wide_pick_kernel: no read-back; parallel fp32 sums)."""
        from . import infer_core

        ids_in = np.asarray(text_ids)
        items, nb, nd = ids_in.shape[0], int(num_beams), 2 * int(num_beams)
        if uniforms is None:
            uniforms = np.random.default_rng(seed).random((max_gen, items, nd), dtype=np.float32)
        u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1, items, nd)
        stop, start = self.ccfg.stop_mel_token, self.ccfg.start_mel_token
        hist = np.empty((items * nb, max_gen), dtype=np.int32)
        scores = np.empty(items * nb, dtype=np.float32)
        done = np.empty(items, dtype=np.int32)
        step = C.c_int()
        self._ck(self.lib.itts_gpt_set_host_sampling(self.h, 1), "gpt_set_host_sampling")
        try:
            self.set_beam_sample(nb, top_k, top_p, temperature, None, do_sample=True, length_penalty=length_penalty,
                                 num_return_sequences=num_return_sequences, host=True)
            self.prefill(cond, text_ids, max_gen, repetition_penalty, suppress_stop)
            while True:
                self._ck(self.lib.itts_gpt_beam_state(self.h, hist.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p),
                                                     done.ctypes.data_as(C.c_void_p), C.byref(step), self._s()), "gpt_beam_state")
                k = step.value
                if k >= max_gen or done.all():
                    break
                lg = np.empty((items * nb, self.ccfg.number_mel_codes), dtype=np.float32)
                self._ck(self.lib.itts_gpt_fetch(self.h, None, lg.ctypes.data_as(C.c_void_p), self._s()), "gpt_fetch")
                psc, ptok, pbeam = infer_core.host_beam_step(lg, hist, k, scores, done, nb, float(repetition_penalty), float(temperature),
                                                             top_k, top_p, float(typical_mass or 0.0), u[k], stop, bool(suppress_stop),
                                                             start)
                self._ck(self.lib.itts_gpt_commit_beams(self.h, psc.ctypes.data_as(C.c_void_p), ptok.ctypes.data_as(C.c_void_p),
                                                       pbeam.ctypes.data_as(C.c_void_p), self._s()), "gpt_commit_beams")
                if k + 1 >= max_gen:
                    break
                self.decode(1)
            step2, _ = self.status()
            codes = self.fetch()[:, :step2].astype(np.int64)
            self._exit()
        finally:
            self.set_beam_sample(1)
            self._ck(self.lib.itts_gpt_set_host_sampling(self.h, 0), "gpt_set_host_sampling")
        n = 0
        for row in codes:
            hit = np.nonzero(row == stop)[0]
            n = max(n, int(hit[0]) + 1 if len(hit) else step2)
        return codes[:, :n]

    def latent(self, cond: torch.Tensor, text_ids: np.ndarray, codes: np.ndarray) -> torch.Tensor:
        """-> latent [1, T, D] engine dtype."""
        t = np.ascontiguousarray(text_ids, dtype=np.int32).reshape(-1)
        c = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
        cond = cond.to(device=self.device, dtype=torch.float32).contiguous().view(-1, self.ccfg.model_dim)
        out = torch.empty(1, c.shape[0], self.ccfg.model_dim, dtype=self.tdt, device=self.device)
        self._enter()
        self._ck(self.lib.itts_gpt_latent(self.h, cond.data_ptr(), t.ctypes.data_as(C.c_void_p), t.shape[0],
                                         c.ctypes.data_as(C.c_void_p), c.shape[0], out.data_ptr(), self._s()), "gpt_latent")
        self._exit()
        return out

    def latent_batch(self, cond: torch.Tensor, texts, codes, cond_index=None) -> List[torch.Tensor]:
        """Several sentences in one pass -> list of latents [1, T_i, D] (views of one buffer).  cond_index (optional, one int per
        sentence): cond holds several conditioning blocks [n_cond, latents, D] and sentence i reads block cond_index[i] - several
        voices in one pass, each sentence with the bits of the pass over its own voice alone."""
        ts = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in texts]
        cs = [np.ascontiguousarray(c, dtype=np.int32).reshape(-1) for c in codes]
        tl = np.asarray([t.shape[0] for t in ts], dtype=np.int32)
        cl = np.asarray([c.shape[0] for c in cs], dtype=np.int32)
        tcat, ccat = np.concatenate(ts), np.concatenate(cs)
        cond = cond.to(device=self.device, dtype=torch.float32).contiguous().view(-1, self.ccfg.model_dim)
        out = torch.empty(int(cl.sum()), self.ccfg.model_dim, dtype=self.tdt, device=self.device)
        self._enter()
        if cond_index is None:
            self._ck(self.lib.itts_gpt_latent_batch(self.h, cond.data_ptr(), tcat.ctypes.data_as(C.c_void_p),
                                                   tl.ctypes.data_as(C.c_void_p), ccat.ctypes.data_as(C.c_void_p),
                                                   cl.ctypes.data_as(C.c_void_p), len(ts), out.data_ptr(), self._s()),
                    "gpt_latent_batch")
        else:
            ci = np.ascontiguousarray(cond_index, dtype=np.int32).reshape(-1)
            n_cond, rem = divmod(cond.shape[0], self.ccfg.cond_latents)
            if rem or ci.shape[0] != len(ts):
                raise ValueError(f"latent_batch: cond {tuple(cond.shape)} / {ci.shape[0]} indices for {len(ts)} sentences")
            self._ck(self.lib.itts_gpt_latent_batch_cond(self.h, cond.data_ptr(), ci.ctypes.data_as(C.c_void_p), n_cond,
                                                        tcat.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p),
                                                        ccat.ctypes.data_as(C.c_void_p), cl.ctypes.data_as(C.c_void_p), len(ts),
                                                        out.data_ptr(), self._s()), "gpt_latent_batch_cond")
        self._exit()
        res, o = [], 0
        for n in cl:
            res.append(out[o:o + int(n)].unsqueeze(0))
            o += int(n)
        return res

    def latent_packed(self, cond: torch.Tensor, texts, codes, cond_index=None, max_tokens=None) -> List[torch.Tensor]:
        """latent_batch on PACKED rows (itts_gpt_latent_packed): the tokens of all sentences back to back, no pad rows, attention
        per sentence from its own key 0, no K split, the GEMM family not chosen by the row count - a sentence's latent has the
        same bits alone, with any companions, in any order and in any chunking.  Runs in chunks of at most 128 sentences and
        max_tokens token rows (infer_core.packed_chunks; None: infer_core.PACKED_MAX_TOKENS).  cond / cond_index as latent_batch.
        -> list of latents [1, T_i, D] (views of one buffer)."""
        from . import infer_core

        ts = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in texts]
        cs = [np.ascontiguousarray(c, dtype=np.int32).reshape(-1) for c in codes]
        if not ts or len(ts) != len(cs):
            raise ValueError(f"latent_packed: {len(ts)} texts / {len(cs)} code rows")
        cond = cond.to(device=self.device, dtype=torch.float32).contiguous().view(-1, self.ccfg.model_dim)
        n_cond, rem = divmod(cond.shape[0], self.ccfg.cond_latents)
        ci = None
        if cond_index is not None:
            ci = np.ascontiguousarray(cond_index, dtype=np.int32).reshape(-1)
            if ci.shape[0] != len(ts):
                raise ValueError(f"latent_packed: {ci.shape[0]} indices for {len(ts)} sentences")
        if rem or n_cond < 1:
            raise ValueError(f"latent_packed: cond {tuple(cond.shape)} is not a whole number of [{self.ccfg.cond_latents}, D] blocks")
        cl = [int(c.shape[0]) for c in cs]
        rows = [self.ccfg.cond_latents + int(t.shape[0]) + 2 + n + 2 for t, n in zip(ts, cl)]
        out = torch.empty(sum(cl), self.ccfg.model_dim, dtype=self.tdt, device=self.device)
        starts = np.concatenate([[0], np.cumsum(cl)]).astype(np.int64)
        es = out.element_size() * self.ccfg.model_dim
        self._enter()
        for chunk in infer_core.packed_chunks(rows, max_tokens or infer_core.PACKED_MAX_TOKENS):
            tl = np.asarray([ts[i].shape[0] for i in chunk], dtype=np.int32)
            kl = np.asarray([cl[i] for i in chunk], dtype=np.int32)
            tcat, ccat = np.concatenate([ts[i] for i in chunk]), np.concatenate([cs[i] for i in chunk])
            cc = None if ci is None else np.ascontiguousarray(ci[chunk])
            self._ck(self.lib.itts_gpt_latent_packed(self.h, cond.data_ptr(), None if cc is None else cc.ctypes.data_as(C.c_void_p), n_cond,
                                                    tcat.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p),
                                                    ccat.ctypes.data_as(C.c_void_p), kl.ctypes.data_as(C.c_void_p), len(chunk),
                                                    out.data_ptr() + int(starts[chunk[0]]) * es, self._s()), "gpt_latent_packed")
        self._exit()
        return [out[int(starts[i]):int(starts[i + 1])].unsqueeze(0) for i in range(len(cl))]

    def latent_stream(self, cond: torch.Tensor, texts, max_codes: int, cond_index=None) -> "LatentStream":
        """The INCREMENTAL packed latent pass (itts_gpt_latent_stream_*; opt-in): the sentences of latent_packed opened together and
        fed their codes in pieces.  -> an object with .append(list of code arrays, one per sentence, empty = leave it alone) ->
        list of latents [1, n_i, D] for the codes just given, and .close(); also a context manager.  After any sequence of appends
        the rows delivered so far are, bit for bit, the first rows of latent_packed over the final codes.  The engine keeps the
        K/V history of every computed row from here to close(); one stream per engine.  cond / cond_index as latent_batch;
        max_codes: the most codes any sentence will be given."""
        return LatentStream(self, cond, texts, max_codes, cond_index)

    def bigvgan_stream(self, spk: torch.Tensor, chunk_frames: int = 1, first_chunk_frames: Optional[int] = None) -> "VocoderStream":
        """Streaming vocoder for one sentence of one voice (spk [E] or [1, E]): an object with .push(latent_frames [1, n, D] or
        [n, D], last=False) -> wav fp32 [1, 1, m * up].  chunk_frames / first_chunk_frames: a push returns nothing (and runs nothing)
        until that many frames are final (infer_core.StreamWindow; 1 = everything that is final, at every push).  Every push runs bigvgan_packed over one window - the frames not yet sent
        plus R = infer_core.vocoder_reach(..) frames of context on either side - and returns only samples whose frames lie R away
        from an artificial window edge, so everything returned is final; the concatenation over the pushes (the last one with
        last=True) equals bigvgan_packed([whole latent], spk)[0] bit for bit.  No kernel of its own."""
        return VocoderStream(self, spk, chunk_frames, first_chunk_frames)

    def vocoder_reach(self) -> int:
        """infer_core.vocoder_reach over this engine's generator: the one-sided reach R of the whole vocoder in latent frames."""
        from . import infer_core

        c = self.ccfg
        nu, nr, nd = int(c.bv_num_up), int(c.bv_num_res), int(c.bv_num_dil)
        return infer_core.vocoder_reach(list(c.bv_up_rates)[:nu], list(c.bv_up_kernels)[:nu], list(c.bv_res_kernels)[:nr],
                                        [list(c.bv_res_dils[j])[:nd] for j in range(nr)])

    def bigvgan(self, latent: torch.Tensor, spk: torch.Tensor) -> torch.Tensor:
        """latent [B, T, D], spk [B, E] -> wav fp32 [B, 1, T*up]."""
        lat = self.to_act(latent)
        B, T, _ = lat.shape
        spk = spk.to(device=self.device, dtype=torch.float32).contiguous().view(B, -1)
        out = torch.empty(B, 1, T * self.up_total, dtype=torch.float32, device=self.device)
        self._enter()
        self._join_side()
        self._ck(self.lib.itts_bigvgan(self.h, lat.data_ptr(), spk.data_ptr(), B, T, out.data_ptr(), self._s()), "bigvgan")
        self._exit()
        lat.record_stream(self.stream)
        spk.record_stream(self.stream)
        return out

    def dvae_encode(self, mel_bct: torch.Tensor) -> np.ndarray:
        """DiscreteVAE.get_codebook_indices: mel [B, channels, T] (reference layout) -> codes int64 [B, T']."""
        mel = self.to_act(mel_bct.transpose(1, 2))
        B, T, _ = mel.shape
        Tc = _dvae_code_len(T, self.ccfg.dv_layers)
        codes = np.empty((B, Tc), dtype=np.int32)
        self._enter()
        self._ck(self.lib.itts_dvae_encode(self.h, mel.data_ptr(), B, T, codes.ctypes.data_as(C.c_void_p), self._s()), "dvae_encode")
        self._exit()
        return codes.astype(np.int64)

    def bigvgan_ragged(self, lats: List[torch.Tensor], spk: torch.Tensor) -> List[torch.Tensor]:
        """One vocoder pass over latents [1, T_i, D] of unequal length (itts_bigvgan_ragged): they are packed into a zero-padded
        [B, Tmax, D] batch with their lengths beside it; every tensor a convolution reads is kept zero behind a row's own end
        and every Activation1d ends its signal there, so each row is the waveform of its latent run alone.  spk [E], [1, E]
        (shared) or [B, E].  -> wavs fp32 [1, 1, T_i * up], in the order of lats."""
        B = len(lats)
        lens = np.asarray([int(l.shape[1]) for l in lats], dtype=np.int32)
        T = int(lens.max())
        D = int(lats[0].shape[2])
        lat = torch.zeros(B, T, D, dtype=self.tdt, device=self.device)
        for b, l in enumerate(lats):
            lat[b, :int(lens[b])] = l[0].to(device=self.device, dtype=self.tdt)
        spk = spk.to(device=self.device, dtype=torch.float32).reshape(-1, spk.shape[-1])
        spk = (spk.expand(B, -1) if spk.shape[0] == 1 else spk).contiguous()
        assert spk.shape[0] == B, (spk.shape, B)
        out = torch.empty(B, 1, T * self.up_total, dtype=torch.float32, device=self.device)
        self._enter()
        self._join_side()
        self._ck(self.lib.itts_bigvgan_ragged(self.h, lat.data_ptr(), spk.data_ptr(), B, T, lens.ctypes.data_as(C.c_void_p),
                                              out.data_ptr(), self._s()), "bigvgan_ragged")
        self._exit()
        lat.record_stream(self.stream)
        spk.record_stream(self.stream)
        return [out[b:b + 1, :, :int(lens[b]) * self.up_total] for b in range(B)]

    def bigvgan_packed_gap(self) -> int:
        """Zero frames a packed sentence needs behind its signal (infer_core.packed_vocoder_gap over this engine's config)."""
        from . import infer_core

        c = self.ccfg
        nu, nr, nd = int(c.bv_num_up), int(c.bv_num_res), int(c.bv_num_dil)
        return infer_core.packed_vocoder_gap(list(c.bv_up_rates)[:nu], list(c.bv_up_kernels)[:nu], list(c.bv_res_kernels)[:nr],
                                             [list(c.bv_res_dils[j])[:nd] for j in range(nr)])

    def bigvgan_packed(self, lats: List[torch.Tensor], spk: torch.Tensor, max_frames: Optional[int] = None) -> List[torch.Tensor]:
        """Vocoder over latents [1, T_i, D] back to back as ONE item (itts_bigvgan_packed; opt-in): no padding to a common length -
        each sentence is followed by bigvgan_packed_gap() zero frames, the reach of the widest convolution - no K split and every
        kernel family picked without looking at the row count, so a sentence's samples are the same bits alone, with any companions
        (of any voice), in any order and in any chunking.  spk [E], [1, E] (shared) or [n, E], one voice per sentence.
        max_frames: the frame budget of one pass (infer_core.packed_vocoder_plan; default PACKED_VOCODER_MAX_FRAMES).
        -> wavs fp32 [1, 1, T_i * up], in the order of lats."""
        from . import infer_core

        n = len(lats)
        if n == 0:
            return []  # as bigvgan_grouped, which it stands in for
        lens = [int(l.shape[1]) for l in lats]
        D = int(lats[0].shape[2])
        spk = spk.to(device=self.device, dtype=torch.float32).reshape(-1, spk.shape[-1])
        if spk.shape[0] not in (1, n):
            raise ValueError(f"bigvgan_packed: {spk.shape[0]} speaker embeddings for {n} latents (one, or one per latent)")
        spk = (spk.expand(n, -1) if spk.shape[0] == 1 else spk).contiguous()
        gap = self.bigvgan_packed_gap()
        chunks, offsets, frames = infer_core.packed_vocoder_plan(lens, gap, max_frames or infer_core.PACKED_VOCODER_MAX_FRAMES)
        res: List[Optional[torch.Tensor]] = [None] * n
        passes = []  # the operands of every pass, made on the caller's stream before the engine's stream starts to wait for it
        for sel, off, tot in zip(chunks, offsets, frames):
            lat = torch.zeros(tot, D, dtype=self.tdt, device=self.device)
            for j, i in enumerate(sel):
                lat[off[j]:off[j] + lens[i]] = lats[i][0].to(device=self.device, dtype=self.tdt)
            sp = spk[sel[0]:sel[-1] + 1].contiguous()  # (chunks are consecutive runs)
            out = torch.empty(tot * self.up_total, dtype=torch.float32, device=self.device)
            passes.append((sel, off, lat, sp, out))
        self._enter()
        self._join_side()
        for sel, off, lat, sp, out in passes:
            offs = np.asarray(off, dtype=np.int32)
            ln = np.asarray([lens[i] for i in sel], dtype=np.int32)
            self._ck(self.lib.itts_bigvgan_packed(self.h, lat.data_ptr(), sp.data_ptr(), offs.ctypes.data_as(C.c_void_p),
                                                  ln.ctypes.data_as(C.c_void_p), len(sel), out.data_ptr(), self._s()), "bigvgan_packed")
            lat.record_stream(self.stream)
            sp.record_stream(self.stream)
            for j, i in enumerate(sel):
                res[i] = out[off[j] * self.up_total:(off[j] + lens[i]) * self.up_total].view(1, 1, -1)
        self._exit()
        return res

    def bigvgan_grouped(self, lats: List[torch.Tensor], spk: torch.Tensor, ragged: bool = False,
                        max_pad: float = 0.1) -> List[torch.Tensor]:
        """Vocoder over several sentences: latents [1, T_i, D] of EQUAL length share one batched launch sequence (rows of
        a batch are independent, so each result equals its batch-1 run).  spk: one embedding [E] / [1, E] for all of them, or
        [n, E], one per latent (several voices in one pass); ragged lengths cannot be padded - the convs
        would see conv_pre(0) = bias instead of zero "same" padding - and go in groups of their own.
        ragged=True (opt-in): rows of unequal length share a pass too (bigvgan_ragged, which masks what plain padding gets
        wrong), grouped by infer_core.ragged_groups so that at most max_pad of a batch's frames are padding; a group of one or
        of equal lengths runs as above.  Same shapes in the same order either way.  max_pad = 0.1 is the best of the three
        values tools/bench_ragged_vocoder.py measured (64 latents of 275 .. 544 frames, bf16, profiles/ragged_vocoder.txt: 1.81 x
        the 64 batch-1 runs at 0.1, 1.64 x at 0.25, 1.65 x at 0.5 - more padding is more frames computed)."""
        cap = max(1, int(self.ccfg.max_batch))
        spk = spk.reshape(-1, spk.shape[-1])
        if spk.shape[0] not in (1, len(lats)):
            raise ValueError(f"bigvgan_grouped: {spk.shape[0]} speaker embeddings for {len(lats)} latents (one, or one per latent)")

        def spk_of(sel):  # [len(sel), E]: the one embedding for every row, or each latent's own
            return (spk.expand(len(sel), -1) if spk.shape[0] == 1 else spk[list(sel)]).contiguous()

        if ragged:
            from . import infer_core

            res: List[Optional[torch.Tensor]] = [None] * len(lats)
            lens = [int(l.shape[1]) for l in lats]
            for sel in infer_core.ragged_groups(lens, max_pad, cap):
                sub = [lats[i] for i in sel]
                if len({lens[i] for i in sel}) == 1:
                    wav = self.bigvgan(torch.cat(sub, 0), spk_of(sel))
                    wavs = [wav[j:j + 1] for j in range(len(sel))]
                else:
                    wavs = self.bigvgan_ragged(sub, spk_of(sel))
                for i, w in zip(sel, wavs):
                    res[i] = w
            return res
        groups: Dict[int, List[int]] = {}
        for i, l in enumerate(lats):
            groups.setdefault(int(l.shape[1]), []).append(i)
        out: List[Optional[torch.Tensor]] = [None] * len(lats)
        for T, idx in groups.items():
            for lo in range(0, len(idx), cap):
                sel = idx[lo:lo + cap]
                wav = self.bigvgan(torch.cat([lats[i] for i in sel], 0), spk_of(sel))
                for j, i in enumerate(sel):
                    out[i] = wav[j:j + 1]
        return out

    def dvae_decode(self, codes: np.ndarray) -> torch.Tensor:
        """codes [B, T] -> mel [B, channels, 4T] (reference layout), engine dtype."""
        c = np.ascontiguousarray(codes, dtype=np.int32)
        B, T = c.shape
        ch = self.ccfg.dv_channels
        up = 2 ** self.ccfg.dv_layers
        out = torch.empty(B, T * up, ch, dtype=self.tdt, device=self.device)
        self._enter()
        self._ck(self.lib.itts_dvae_decode(self.h, c.ctypes.data_as(C.c_void_p), B, T, out.data_ptr(), self._s()), "dvae_decode")
        self._exit()
        return out.transpose(1, 2)


class LatentStream:
    """Engine.latent_stream's object: the engine-side stream state from construction to close()."""

    def __init__(self, eng: Engine, cond: torch.Tensor, texts, max_codes: int, cond_index=None):
        self.eng = eng
        ts = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in texts]
        if not ts:
            raise ValueError("latent_stream: no texts")
        D = eng.ccfg.model_dim
        self.cond = cond.to(device=eng.device, dtype=torch.float32).contiguous().view(-1, D)  # kept: the engine reads it at every first append
        n_cond, rem = divmod(self.cond.shape[0], eng.ccfg.cond_latents)
        if rem or n_cond < 1:
            raise ValueError(f"latent_stream: cond {tuple(cond.shape)} is not a whole number of [{eng.ccfg.cond_latents}, D] blocks")
        ci = None
        if cond_index is not None:
            ci = np.ascontiguousarray(cond_index, dtype=np.int32).reshape(-1)
            if ci.shape[0] != len(ts):
                raise ValueError(f"latent_stream: {ci.shape[0]} indices for {len(ts)} sentences")
        self.n = len(ts)
        tl = np.asarray([t.shape[0] for t in ts], dtype=np.int32)
        tcat = np.concatenate(ts)
        self.open = False
        eng._enter()
        eng._ck(eng.lib.itts_gpt_latent_stream_open(eng.h, self.cond.data_ptr(), None if ci is None else ci.ctypes.data_as(C.c_void_p), n_cond,
                                                    tcat.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p), self.n, int(max_codes),
                                                    eng._s()), "gpt_latent_stream_open")
        eng._exit()
        self.open = True

    def append(self, codes) -> List[torch.Tensor]:
        eng = self.eng
        cs = [np.ascontiguousarray(c, dtype=np.int32).reshape(-1) for c in codes]
        if len(cs) != self.n:
            raise ValueError(f"latent_stream.append: {len(cs)} code arrays for {self.n} sentences")
        counts = np.asarray([c.shape[0] for c in cs], dtype=np.int32)
        ccat = np.concatenate(cs) if int(counts.sum()) else np.zeros(1, dtype=np.int32)
        out = torch.empty(int(counts.sum()), eng.ccfg.model_dim, dtype=eng.tdt, device=eng.device)
        eng._enter()
        eng._ck(eng.lib.itts_gpt_latent_stream_append(eng.h, ccat.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                      out.data_ptr() if out.numel() else self.cond.data_ptr(), eng._s()),
                "gpt_latent_stream_append")
        eng._exit()
        starts = np.concatenate([[0], np.cumsum(counts)])
        return [out[int(starts[i]):int(starts[i + 1])].unsqueeze(0) for i in range(self.n)]

    def close(self):
        if self.open:
            self.open = False
            self.eng._ck(self.eng.lib.itts_gpt_latent_stream_close(self.eng.h), "gpt_latent_stream_close")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VocoderStream:
    """Engine.bigvgan_stream's object.  State: the latent frames from R in front of the first frame not yet sent (`lo` = that
    buffer's first frame index) and how many frames were sent."""

    def __init__(self, eng: Engine, spk: torch.Tensor, chunk_frames: int = 1, first_chunk_frames: Optional[int] = None):
        from . import infer_core

        self.eng = eng
        self.spk = spk.to(device=eng.device, dtype=torch.float32).reshape(1, -1)
        self.R = eng.vocoder_reach()
        self.plan = infer_core.StreamWindow(self.R, chunk_frames, first_chunk_frames)
        self.buf = None  # [n, D]: frames [plan.lo, plan.have)
        self.done = False

    def push(self, latent: Optional[torch.Tensor], last: bool = False) -> torch.Tensor:
        """latent [1, n, D] / [n, D] (n >= 0; None = nothing new) -> the samples that became final, fp32 [1, 1, m * up]"""
        eng = self.eng
        if self.done:
            raise ValueError("bigvgan_stream.push: the stream has ended (last=True was given)")
        D = eng.ccfg.model_dim
        new = torch.empty(0, D, dtype=eng.tdt, device=eng.device) if latent is None else eng.to_act(latent).reshape(-1, D)
        self.buf = new if self.buf is None else torch.cat([self.buf, new], 0)
        lo, a, b = self.plan.push(int(new.shape[0]), last)  # the window starts at frame lo; frames [a, b) become final
        self.done = bool(last)
        up = eng.up_total
        if b <= a:
            return torch.empty(1, 1, 0, dtype=torch.float32, device=eng.device)
        wav = eng.bigvgan_packed([self.buf.unsqueeze(0)], self.spk)[0]
        out = wav[:, :, (a - lo) * up:(b - lo) * up].clone()
        keep = self.plan.lo - lo  # frames the window no longer needs
        if keep > 0:
            self.buf = self.buf[keep:]
        return out


def _warn_downgrade(err):
    import logging
    import warnings

    msg = ("itts_hip: the persistent decode engine timed out on a hand-off (one process per GPU is required, INTEGRATION.md); "
           f"this engine now decodes on the five-launches-per-block path and the utterance is generated again: {err}")
    logging.getLogger("itts_hip").warning(msg)
    warnings.warn(msg, RuntimeWarning, stacklevel=3)


def _dvae_code_len(T: int, layers: int) -> int:
    for _ in range(layers):
        T = (T + 1) // 2
    return T


def build_engine(cfg, dtype: str = "bf16", device: str = "cuda:0", seed: int = 1234, parts=("gpt", "bigvgan", "dvae"),
                 state_dicts: Optional[dict] = None, max_batch: int = 64, gpt_fp8: str = "", engine_fp8: bool = False,
                 kv_fp8: bool = False, engine_kv_fp8: bool = False, retire_beams: bool = False) -> Engine:
    """Engine with synthetic (PRNG) or supplied reference-layout state dicts.  gpt_fp8: "" = plain weights;
    "fp8" = GPT projections quantised to e4m3 (power-of-two row scales) with the fp8 bytes used by the decode GEMV;
    "dequant" = the same quantised model but every kernel reads its bf16 dequantisation (the fp8 path's reference).
    engine_fp8: Engine.set_engine_fp8(True) - the fp8 model's small-batch decode steps on the persistent decode engine.
    kv_fp8: Engine.set_kv_fp8(True) - the decode steps' K/V cache as fp8-e4m3 bytes (16-bit engines).
    engine_kv_fp8: Engine.set_engine_kv_fp8(True) - with an fp8 cache the small-batch decode steps stay on the persistent engine.
    retire_beams: Engine.set_retire_beams(True) - retire_rows() also retires the finished groups of a beam generation."""
    from . import pack, synth

    eng = Engine(cfg, dtype, device, max_batch)
    sds = state_dicts or {}
    if "gpt" in parts:
        packed = pack.pack_gpt(sds.get("gpt") or synth.gpt_state_dict(cfg, seed), cfg)
        if gpt_fp8:
            packed = pack.quantize_gpt_fp8(packed, keep_bytes=(gpt_fp8 == "fp8"))
        eng.load_packed(packed)
    if "bigvgan" in parts:
        eng.load_packed(pack.pack_bigvgan(sds.get("bigvgan") or synth.bigvgan_state_dict(cfg, seed), cfg))
    if "dvae" in parts:
        eng.load_packed(pack.pack_dvae(sds.get("dvae") or synth.dvae_state_dict(cfg, seed), cfg))
    eng.finalize()
    if engine_fp8:
        eng.set_engine_fp8(True)
    if kv_fp8:
        eng.set_kv_fp8(True)
    if engine_kv_fp8:
        eng.set_engine_kv_fp8(True)
    if retire_beams:
        eng.set_retire_beams(True)
    return eng
