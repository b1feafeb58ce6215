import os
import sys

from . import _lib, launch
from .phyloligo import get_cmd, launch_plan, main, refuse

# One parse (get_cmd: --help and a malformed command line end here, once), one decision (launch_plan), both before anything has
# touched torch or the HIP runtime.
_params = get_cmd()
_refused, _gpus, _needs_torch = launch_plan(_params, os.environ)
if launch.needs_launcher(_gpus):
    # --gpus N > 1: this process only starts one rank per GPU (python -m torch.distributed.run ... -m phyloligo_amd <same
    # arguments>) and waits for them - the reference fans out to its own workers the same way (bin/phyloligo.py:386-390).
    # What the ranks would refuse is refused here, before any is started.  A failed launch is reported; the reference's exit
    # status 0 (:1075) is kept for a job that ran.
    refuse(_refused)
    sys.exit(launch.spawn_ranks(_gpus, ["-m", "phyloligo_amd"], sys.argv[1:],
                                timeout_s=float(os.environ.get("PO_CLI_LAUNCH_TIMEOUT", "0")) or None))

_lib.PREFER_NO_TORCH = not _needs_torch      # one process, one GPU, no matrix kept in a torch tensor: numpy + the host-pointer
main(params=_params)                         # entry points of the C ABI are enough
sys.exit(0)      # the reference always exits 0 (phyloligo.py:1075)
