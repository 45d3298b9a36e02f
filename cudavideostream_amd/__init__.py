"""cudavideostream_amd -- MI355X (gfx950) implementation of the frame-differencing + filter hot
path of MatteoBattilana/CUDAVideoStream behind the reference's own CUDACore call surface.

  csrc/      hand-written HIP kernels + the C-ABI (include/mi355diff.h) -> libmi355diff.so
  compat/    C++ `diff::cuda::CUDACore` drop-in that the reference server.cpp links against
  core.py    the same surface for Python callers (ctypes over the C-ABI)
  synth.py   deterministic synthetic frames
"""
from .core import CHARS_STR, LR_THRESHOLDS, CUDACore, PinnedArray  # noqa: F401
from .core import activity_cells, cwire_apply_host, cwire_budget_entries, cwire_bytes_max, cwire_frame_bytes  # noqa: F401
from .core import cwire_despeckle_host  # noqa: F401
from .core import cwire_check_host, state_digest_host, state_tiles, thumb_cwire_host, wall_thumb_size  # noqa: F401
from .core import cwire_split_bytes_max, cwire_split_host, cwire_split_pieces_max  # noqa: F401
from .core import cwire_fec_groups_max, cwire_fec_host, cwire_fec_repair_host  # noqa: F401
from .core import cwire_runs_bytes_max, cwire_runs_decode_host, cwire_runs_encode_host, cwire_runs_frame_bytes  # noqa: F401
from .lib import RUNS_ALWAYS, RUNS_FORM_COMPACT, RUNS_FORM_RUNS, RUNS_WHERE_SMALLER  # noqa: F401
from .lib import FEC_ABSENT, FEC_BAD_HEADER, FEC_BAD_TAIL  # noqa: F401
from .lib import CWIRE_BAD_CODES, CWIRE_BAD_ESCAPE, CWIRE_BAD_HEADER, CWIRE_BAD_PAD, CWIRE_BAD_RANGE  # noqa: F401
from . import lib  # noqa: F401
