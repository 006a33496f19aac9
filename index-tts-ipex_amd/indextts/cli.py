"""`indextts` console entry (/root/reference/indextts/cli.py:7-70): text + voice prompt -> wav file."""
import argparse
import os
import sys


def build_parser():
    p = argparse.ArgumentParser(description="IndexTTS Command Line (MI355X HIP engine)")
    p.add_argument("text", type=str, help="Text to be synthesized")
    p.add_argument("-v", "--voice", type=str, required=True, help="Path to the audio prompt file (wav format)")
    p.add_argument("-o", "--output_path", type=str, default="gen.wav")
    p.add_argument("-c", "--config", type=str, default="checkpoints/config.yaml")
    p.add_argument("--model_dir", type=str, default="checkpoints")
    p.add_argument("--fp16", action="store_true", default=True, help="bf16 throughput engine (default)")
    p.add_argument("--fp32", action="store_true", help="fp32 parity engine")
    p.add_argument("-f", "--force", action="store_true", default=False)
    p.add_argument("-d", "--device", type=str, default=None)
    p.add_argument("--wide-sampler", choices=("device", "host"), default=None,
                   help="where sampling with one beam and top_k = 0 or > 128 picks its tokens: host (torch's arithmetic, one sync per "
                        "token; the default) or device (the whole-vocabulary HIP sampler); unset: ITTS_WIDE_SAMPLER")
    p.add_argument("--wide-beam-sampler", choices=("device", "host"), default=None,
                   help="the same choice with several beams (beam_sample with top_k = 0 or > 128): host (the default) or device (the "
                        "whole-vocabulary HIP beam sampler); unset: ITTS_WIDE_BEAM_SAMPLER")
    p.add_argument("--gpt-fp8", action="store_true", default=False,
                   help="store the GPT weights as fp8-e4m3 (bfloat16 engine; the decode steps stream the fp8 bytes)")
    p.add_argument("--kv-fp8", action="store_true", default=False,
                   help="keep the K/V cache of the GPT decode steps as fp8-e4m3 bytes (16-bit engines; half the cache bytes per step)")
    p.add_argument("--engine-kv-fp8", action="store_true", default=False,
                   help="with --kv-fp8: keep the 1 - 6 row decode steps on the persistent decode engine, which reads the fp8 cache itself")
    p.add_argument("--retire-rows", type=float, default=None, metavar="R",
                   help="batched generations retire their finished rows whenever unfinished <= R * running rows (0 < R <= 1; more "
                        "than 6 rows); unset: ITTS_RETIRE_ROWS, else off")
    p.add_argument("--retire-beams", action="store_true", default=None,
                   help="with --retire-rows: beam generations (the default, num_beams=3) retire the rows of their finished sentences "
                        "too; unset: ITTS_RETIRE_BEAMS, else off")
    p.add_argument("--ragged-vocoder", action="store_true", default=False,
                   help="batched synthesis (IndexTTS.infer_batch): sentences of unequal length share vocoder passes; "
                        "ITTS_RAGGED_VOCODER=0 / 1 overrides")
    p.add_argument("--admit-rows", action="store_true", default=False,
                   help="batched synthesis (IndexTTS.infer_batch with mixed batches, ITTS_MIXED_BATCH=1): finished decode rows are "
                        "refilled from the waiting sentences; ITTS_ADMIT_ROWS=0 / 1 overrides")
    p.add_argument("--admit-beams", action="store_true", default=False,
                   help="with --admit-rows: beam groups (the default, num_beams=3) are refilled too, a finished sentence's rows take "
                        "the next waiting sentence; ITTS_ADMIT_BEAMS=0 / 1 overrides")
    p.add_argument("--packed-latent", action="store_true", default=False,
                   help="batched synthesis (IndexTTS.infer_batch): the latent pass runs on packed rows without padding, one pass per "
                        "decode group under mixed batches; ITTS_PACKED_LATENT=0 / 1 overrides")
    p.add_argument("--packed-vocoder", action="store_true", default=False,
                   help="batched synthesis (IndexTTS.infer_batch): the vocoder runs over the sentences back to back as one item without "
                        "padding, one pass per decode group under mixed batches; ITTS_PACKED_VOCODER=0 / 1 overrides")
    p.add_argument("--stream", action="store_true", default=False,
                   help="synthesize with IndexTTS.infer_stream (one beam): audio chunks arrive while a sentence still decodes; writes the "
                        "same file and prints the time to the first chunk")
    p.add_argument("--chunk-frames", type=int, default=None, metavar="N",
                   help="with --stream: latent frames per audio chunk (1 frame = 1024 samples); unset: ITTS_STREAM_CHUNK, else the default")
    return p


def stream_to_file(tts, a):
    """--stream: the chunks of infer_stream, written as one wav file; -> seconds to the first chunk"""
    import time

    import numpy as np
    from scipy.io import wavfile

    t0 = time.perf_counter()
    first, parts = None, []
    for _, pcm in tts.infer_stream(audio_prompt=a.voice, text=a.text.strip(), chunk_frames=a.chunk_frames):
        if first is None:
            first = time.perf_counter() - t0
        parts.append(pcm)
    total = time.perf_counter() - t0
    wav = np.concatenate(parts, 0)
    if os.path.isfile(a.output_path):
        os.remove(a.output_path)
    if os.path.dirname(a.output_path):
        os.makedirs(os.path.dirname(a.output_path), exist_ok=True)
    wavfile.write(a.output_path, 24000, wav)
    print(f">> streamed {len(parts)} chunks: first chunk after {first:.3f} s, all after {total:.3f} s; generated audio: {wav.shape[0] / 24000:.2f} s")
    return first


def main():
    p = build_parser()
    a = p.parse_args()
    if not a.text.strip():
        print("ERROR: Text is empty.")
        p.print_help()
        sys.exit(1)
    if not os.path.exists(a.voice):
        print(f"Audio prompt file {a.voice} does not exist.")
        sys.exit(1)
    if not os.path.exists(a.config):
        print(f"Config file {a.config} does not exist.")
        sys.exit(1)
    if os.path.exists(a.output_path) and not a.force:
        print(f"ERROR: Output file {a.output_path} already exists. Use --force to overwrite.")
        sys.exit(1)
    from indextts.infer import IndexTTS

    tts = IndexTTS(cfg_path=a.config, model_dir=a.model_dir, is_fp16=not a.fp32, device=a.device, gpt_fp8=a.gpt_fp8, kv_fp8=a.kv_fp8,
                   wide_sampler=a.wide_sampler, wide_beam_sampler=a.wide_beam_sampler, retire_rows=a.retire_rows,
                   engine_kv_fp8=a.engine_kv_fp8, ragged_vocoder=a.ragged_vocoder, admit_rows=a.admit_rows, retire_beams=a.retire_beams,
                   packed_latent=a.packed_latent, admit_beams=a.admit_beams, packed_vocoder=a.packed_vocoder)
    if a.stream:
        stream_to_file(tts, a)
        return
    tts.infer(audio_prompt=a.voice, text=a.text.strip(), output_path=a.output_path)


if __name__ == "__main__":
    main()
