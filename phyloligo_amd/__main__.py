import os
import sys

from . import _lib, launch


def _gpus_asked(argv):
    """--gpus N / --gpus=N without argparse (the full parser lives behind imports the launcher should not need)"""
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            return argv[i + 1]
        if a.startswith("--gpus="):
            return a.split("=", 1)[1]
    return "1"


try:
    _n = int(_gpus_asked(sys.argv[1:]))
except ValueError:
    _n = 1                               # get_cmd() below reports the malformed value
if _n > 1 and any(a == "--tsne" or a.startswith("--tsne=") for a in sys.argv[1:]):
    # refused before any rank is started (phyloligo._tsne_refused says the same inside a rank)
    sys.stderr.write("Error, --tsne runs on one GPU: an embedding over several ranks (--gpus N > 1) is out of scope\n")
    sys.exit(1)
_sweep = any(a == "--kmedoids-sweep" or a.startswith("--kmedoids-sweep=") for a in sys.argv[1:])
_kmedoids = _sweep or any(a == "--kmedoids" or a.startswith("--kmedoids=") for a in sys.argv[1:])
if _n > 1 and _kmedoids:
    sys.stderr.write("Error, %s runs on one GPU: clustering over several ranks (--gpus N > 1) is out of scope\n"
                     % ("--kmedoids-sweep" if _sweep else "--kmedoids"))
    sys.exit(1)


def _opt(argv, name, default):
    for i, a in enumerate(argv):
        if a == name and i + 1 < len(argv):
            return argv[i + 1]
        if a.startswith(name + "="):
            return a.split("=", 1)[1]
    return default


try:
    _clip = float(_opt(sys.argv[1:], "--clip-percentile", "1")) != 1 or int(_opt(sys.argv[1:], "--min-size", "0")) != 0
except ValueError:
    _clip = False                        # get_cmd() reports the malformed value
if _n > 1 and _clip:
    sys.stderr.write("Error, --clip-percentile / --min-size run on one GPU: a clip over several ranks (--gpus N > 1) is out of scope\n")
    sys.exit(1)
if launch.needs_launcher(_n):
    # --gpus N > 1: this process only starts one rank per GPU (python -m torch.distributed.run ... -m phyloligo_amd <same
    # arguments>) and waits for them - the reference fans out to its own workers the same way (bin/phyloligo.py:386-390).
    # It has touched neither torch nor the HIP runtime.  A failed launch is reported; the reference's exit status 0 (:1075)
    # is kept for a job that ran.
    sys.exit(launch.spawn_ranks(_n, ["-m", "phyloligo_amd"], sys.argv[1:],
                                timeout_s=float(os.environ.get("PO_CLI_LAUNCH_TIMEOUT", "0")) or None))

if int(os.environ.get("WORLD_SIZE", "1")) <= 1 and not _kmedoids and not _clip:      # (--kmedoids and the clip keep the matrix in a torch CUDA tensor)
    _lib.PREFER_NO_TORCH = True      # one process, one GPU: numpy + the host-pointer entry points of the C ABI are enough

from .phyloligo import main  # noqa: E402

main()
sys.exit(0)      # the reference always exits 0 (phyloligo.py:1075)
