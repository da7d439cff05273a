"""CPU: `vid2vid(config_path)` end to end behind a stand-in ffmpeg and a stand-in animate; the ffmpeg commands, `probe_video` and
`annotators_from_config`."""
import json
import os
import shlex
import stat
import sys

import numpy as np
import pytest
from PIL import Image

from vid2vid_util import write_stand_in


def stand_in_animate(calls):
    """ControlAnimatePipeline.animate's contract on the host: a deterministic function of the inputs, the looped-back frames and the
    window's settings."""
    def animate(input_frames, last_output_frames, config):
        calls.append(dict(n=len(input_frames), strength=config["strength"], overlaps=config["overlaps"], epoch=config["epoch"], W=config["W"], H=config["H"],
                          last=None if last_output_frames is None else len(last_output_frames)))
        rng = np.random.default_rng(100 + config["epoch"])
        out = []
        for i, fr in enumerate(input_frames):
            base = rng.integers(0, 256, (config["H"], config["W"], 3), dtype=np.uint8)
            if fr is not None:
                base = (base // 2 + np.asarray(fr) // 2).astype(np.uint8)
            if last_output_frames is not None and i < len(last_output_frames):
                base = (base // 2 + np.asarray(last_output_frames[i]) // 2).astype(np.uint8)
            out.append(Image.fromarray(base))
        return out
    return animate


def _yaml(tmp_path, **over):
    import yaml
    cfg = dict(input_video_path="", output_video_dir=str(tmp_path / "out"), save_frames=0, width=100, height=130, start_time="00:00:01",
               end_time="00:00:00", overlap_strength=0.6, strength=1.0, loop_back_frames=1, do_initial_generation=0, upscale=1, frame_count=4,
               overlap_length=2, seed=5, fps=15, fps_ffmpeg=30, crf=23, total_frames=0)
    cfg.update(over)
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def test_vid2vid_from_a_config_with_stand_ins(tmp_path):
    from controlanimate_amd import vid2vid as V
    ffmpeg = write_stand_in(tmp_path)
    rng = np.random.default_rng(0)
    video = rng.integers(0, 256, (10, 128, 64, 3), dtype=np.uint8)
    np.save(tmp_path / "clip.npy", video)
    cfg_path = _yaml(tmp_path, input_video_path=str(tmp_path / "clip.npy"), save_frames=1)
    calls = []
    run = {}
    out = V.vid2vid(cfg_path, animate=stand_in_animate(calls), ffmpeg_path=ffmpeg, report=run)
    # the size: floored to multiples of 64 and written back as W / H (scripts/vid2vid.py:82-86)
    assert (run["config"]["W"], run["config"]["H"]) == (64, 128) and all((c["W"], c["H"]) == (64, 128) for c in calls)
    # the stopping rule and the emitted counts: 10 frames in windows of 4 with 2 carried -> 2, 2, 2 and the whole last batch
    assert run["emitted"] == [2, 2, 2, 4] and [c["n"] for c in calls] == [4, 4, 4, 4]
    assert [c["strength"] for c in calls] == [1.0, 0.6, 0.6, 0.6] and [c["overlaps"] for c in calls] == [0, 2, 2, 2]
    assert [c["epoch"] for c in calls] == [0, 1, 2, 3] and [c["last"] for c in calls] == [None, 2, 2, 2]
    # the bytes the encoder received == run_windows driven by hand with the same animate
    calls2 = []
    animate = stand_in_animate(calls2)
    wc = V.WindowConfig(frame_count=4, overlap_length=2, strength=1.0, overlap_strength=0.6, loop_back_frames=True)
    by_hand = [np.asarray(f) for w in V.run_windows(
        [Image.fromarray(f) for f in video], lambda b, l, c: animate(b, l, dict(strength=c.strength, overlaps=c.overlaps, epoch=c.epoch, W=64, H=128)), wc)
        for f in w]
    written = np.frombuffer(open(run["output"], "rb").read(), dtype=np.uint8)
    assert written.size == 10 * 128 * 64 * 3 and np.array_equal(written, np.stack(by_hand).reshape(-1))
    assert calls2 == calls
    # the commands: the reader with the reference's eq filter and no end time (00:00:00 means none), the writer at the output size
    reader = json.load(open(str(tmp_path / "clip.npy") + ".argv.json"))
    assert reader == V.ffmpeg_reader_cmd(str(tmp_path / "clip.npy"), 64, 128, 15, "00:00:01", None, ffmpeg, eq="brightness=0.06:saturation=4")[1:]
    assert "-to" not in reader and "eq=brightness=0.06:saturation=4,fps=15,scale=64:128" in reader
    assert json.load(open(run["output"] + ".argv.json")) == V.ffmpeg_writer_cmd(run["output"], 64, 128, 15, 23, ffmpeg)[1:]
    # the post-pass ran, because there is an input video, and its result is what is returned
    assert os.path.basename(out) == "Audio" + os.path.basename(run["output"]) and open(out, "rb").read() == b"post"
    assert json.load(open(out + ".argv.json")) == run["post_pass"][1:]
    # save_frames: the PNGs and info.json from the same host copy
    frames_dir = [d for d in os.listdir(tmp_path / "out") if d.startswith("vid2vid_frames_")]
    assert len(frames_dir) == 1
    names = sorted(os.listdir(tmp_path / "out" / frames_dir[0]))
    assert names == ["{:04d}.png".format(i) for i in range(1, 11)] + ["info.json"]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / frames_dir[0] / "0007.png")), by_hand[6])
    assert json.load(open(tmp_path / "out" / frames_dir[0] / "info.json"))["W"] == 64


def test_vid2vid_text_to_video_stops_at_total_frames_and_draws_a_seed(tmp_path, capsys):
    from controlanimate_amd import vid2vid as V
    ffmpeg = write_stand_in(tmp_path)
    calls = []
    run = {}
    out = V.vid2vid(_yaml(tmp_path, total_frames=6, width=64, height=64, seed=-1), animate=stand_in_animate(calls), ffmpeg_path=ffmpeg, report=run)
    assert run["emitted"] == [2, 4] and out == run["output"] and "post_pass" not in run     # no input video: no post-pass
    assert os.path.getsize(out) == 6 * 64 * 64 * 3
    assert 1 <= run["config"]["seed"] < 2 ** 16 and ">>>> SEED: %d" % run["config"]["seed"] in capsys.readouterr().out


def test_reader_default_is_unchanged_and_the_post_pass_is_the_reference_command():
    from controlanimate_amd import vid2vid as V
    assert V.ffmpeg_reader_cmd("in.mp4", 512, 768, 15) == ["ffmpeg", "-loglevel", "error", "-ss", "00:00:00", "-i", "in.mp4", "-vf",
                                                             "fps=15,scale=512:768", "-f", "rawvideo", "-pix_fmt", "rgb24", "-"]
    # modules/utils.py:43-55 with its arguments filled in, as the shell the reference hands it to splits it
    text = ('/usr/bin/ffmpeg -i tmp/output/Video_a.mp4 -vn -ss 00:00:01 -to 00:00:05 -i tmp/a.mp4 -q:v 0 -crf 23 '
            '-vf "minterpolate=fps=30:mi_mode=mci:mc_mode=aobmc:me_mode=bidir:vsbmc=1"  -shortest -c:v libx264 -preset fast -strict -2 '
            '-fflags shortest -loglevel debug -y "tmp/output/AudioVideo_a.mp4"')
    assert V.ffmpeg_audio_fps_cmd("tmp/output/AudioVideo_a.mp4", "tmp/output/Video_a.mp4", "tmp/a.mp4", 30, 23, "00:00:01", "00:00:05",
                                  "/usr/bin/ffmpeg") == shlex.split(text)


def test_probe_video_reads_ffprobe_json(tmp_path):
    from controlanimate_amd import vid2vid as V
    probe = tmp_path / "ffprobe_stand_in.py"
    probe.write_text(f'#!{sys.executable}\nimport json, sys\nassert sys.argv[-1] == "in.mp4" and "json" in sys.argv\n'
                     'print(json.dumps({"streams": [{"width": 1280, "height": 720, "avg_frame_rate": "30000/1001", "r_frame_rate": "30/1", '
                     '"nb_frames": "N/A", "duration": "2.002"}]}))\n')
    probe.chmod(probe.stat().st_mode | stat.S_IXUSR)
    fps, count, w, h = V.probe_video("in.mp4", str(probe))
    assert (w, h) == (1280, 720) and fps == pytest.approx(29.97, abs=1e-2) and count == pytest.approx(60.0, abs=1e-6)


def test_annotators_from_config_names_the_places_searched(tmp_path, monkeypatch):
    from controlanimate_amd.vid2vid import annotators_from_config
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="no network") as e:
        annotators_from_config(dict(controlnets=["lllyasviel/sd-controlnet-hed"]), None)
    assert os.path.join("models/Annotators", "ControlNetHED.pth") in str(e.value)
    with pytest.raises(FileNotFoundError) as e:
        annotators_from_config(dict(controlnets=["lllyasviel/control_v11p_sd15_openpose"]), None, root=str(tmp_path / "w"))
    assert os.path.join(str(tmp_path / "w"), "body_pose_model.pth") in str(e.value)
    assert annotators_from_config(dict(controlnets=["some/unknown-net"]), None) == {}
    got = annotators_from_config(dict(controlnets=["lllyasviel/sd-controlnet-canny"]), None)
    assert list(got) == ["canny"] and type(got["canny"]).__name__ == "CannyAnnotator"


def test_the_device_route_is_not_in_this_tree(tmp_path):
    from controlanimate_amd import vid2vid as V
    with pytest.raises(NotImplementedError, match="device_frames"):
        V.vid2vid(_yaml(tmp_path, total_frames=6), animate=stand_in_animate([]), device_frames=True)
