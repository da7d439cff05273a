"""GPU: `vid2vid(config_path)` and the command line with the tiny model tree of tests/test_facade_from_files_cpu.py behind a stand-in
ffmpeg: the bytes the encoder receives equal `run_windows` driven by hand with the same pipeline settings, run after run."""
import os

import numpy as np
import pytest
import yaml
from PIL import Image

from test_facade_from_files_cpu import _config, model_tree  # noqa: F401  (fixture)
from vid2vid_util import write_stand_in

pytestmark = pytest.mark.gpu

DEV = "cuda"
WINDOW = dict(frame_count=4, overlap_length=2, overlap_strength=0.5, loop_back_frames=1, scheduler="DDIMScheduler", steps=2, strength=1.0,
              guidance_scale=7.5)


def stack(frames):
    return np.stack([np.asarray(f) for f in frames])


def test_vid2vid_from_a_config_equals_the_window_loop_by_hand(model_tree, tmp_path):  # noqa: F811
    """Three windows of four 64 x 64 frames, overlap 2 at strength 0.5 with loop-back: the chain through the VAE encode of looped-back
    output, colour-matched by ColorMatcher(device), as vid2vid() sets it up."""
    from controlanimate_amd import vid2vid as V
    from controlanimate_amd.color_match import ColorMatcher
    from controlanimate_amd.controlanimate_pipeline import ControlAnimatePipeline
    cfg = _config(model_tree, **WINDOW)
    rng = np.random.default_rng(5)
    frames = [Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8)) for _ in range(8)]
    pipe = ControlAnimatePipeline(cfg)

    def animate(batch, last, c):
        return pipe.animate(batch, last, dict(cfg, frame_count=c.frame_count, L=c.L, strength=c.strength, overlap=c.overlap, overlaps=c.overlaps,
                                              epoch=c.epoch))

    wc = V.WindowConfig(frame_count=4, overlap_length=2, strength=1.0, overlap_strength=0.5, loop_back_frames=True)
    by_hand = [stack(w) for w in V.run_windows(frames, animate, wc, match_colors=ColorMatcher(DEV))]
    assert [len(w) for w in by_hand] == [2, 2, 4] and all(w.std() > 0 for w in by_hand)
    want = np.concatenate(by_hand).reshape(-1)
    del pipe

    ffmpeg = write_stand_in(tmp_path)
    np.save(tmp_path / "clip.npy", stack(frames))
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(dict(cfg, input_video_path=str(tmp_path / "clip.npy"), output_video_dir=str(tmp_path / "out"), ffmpeg_path=ffmpeg,
                                        start_time="00:00:00", end_time="00:00:00", fps=8, fps_ffmpeg=16, crf=20, upscale=1, do_initial_generation=0)))
    run = {}
    out = V.vid2vid(str(path), report=run)
    assert run["emitted"] == [2, 2, 4] and os.path.basename(out) == "Audio" + os.path.basename(run["output"])
    assert np.array_equal(np.frombuffer(open(run["output"], "rb").read(), dtype=np.uint8), want)
    # the command line: a second run writes a second file with the same bytes
    before = set(os.listdir(tmp_path / "out"))
    assert V.main(["--config", str(path)]) == 0
    new = [f for f in set(os.listdir(tmp_path / "out")) - before if f.startswith("Video_") and f.endswith(".mp4")]
    assert len(new) == 1
    assert np.array_equal(np.frombuffer(open(tmp_path / "out" / new[0], "rb").read(), dtype=np.uint8), want)
