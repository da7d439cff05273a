"""A stand-in for ffmpeg, shared by the tests of the vid2vid entry point."""
import stat
import sys


STAND_IN = '''#!{python}
"""A stand-in for ffmpeg: reader mode streams the raw rgb24 frames of an .npy, writer mode stores stdin, the post-pass stores argv."""
import json, sys
import numpy as np
argv = sys.argv[1:]
src = argv[argv.index("-i") + 1]
if "-vn" in argv:
    json.dump(argv, open(argv[-1] + ".argv.json", "w"))
    open(argv[-1], "wb").write(b"post")
elif src == "-":
    json.dump(argv, open(argv[-1] + ".argv.json", "w"))
    open(argv[-1], "wb").write(sys.stdin.buffer.read())
else:
    json.dump(argv, open(src + ".argv.json", "w"))
    sys.stdout.buffer.write(np.load(src).tobytes())
'''


def write_stand_in(tmp_path) -> str:
    path = tmp_path / "ffmpeg_stand_in.py"
    path.write_text(STAND_IN.format(python=sys.executable))
    path.chmod(path.stat().st_mode | stat.S_IXUSR)
    return str(path)
