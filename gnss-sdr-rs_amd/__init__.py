"""gnss-sdr-rs_amd — MI355X-native acquisition + tracking hot path of kewei/gnss-sdr-rs.

The product is the C-ABI shared library built from csrc/ (hand-written HIP for gfx950), declared in
include/gnss_mi355x.h.  This Python package is plumbing around it:
  _lib        ctypes loader (fails loudly when the library is missing; there is no CPU fallback)
  acquisition / tracking / fft   thin mirrors of the reference's Rust API names over the C ABI
  frontend / resample            the digital front-end, and the rate conversion and pulse blanking it leaves out
  excise                         FFT-domain narrowband interference excision (overlap-add filter bank, adaptive per-bin gains)
  ddc                            real-IF int8 down-conversion to complex baseband (exact NCO, the resampler's polyphase filter)
  channelizer                    polyphase filter bank: M sub-bands of one stream (FDMA carriers), and the GLONASS L1OF code
  nuller                         adaptive spatial nulling: A interleaved antennas combined per block with weights from the block's covariance
  stap                           space-time adaptive nulling: the nuller with L taps in time behind every antenna
  beamformer                     one beam per satellite: P constraint rows on stap's stream, one Gram matrix and one factor a block
  lcmv                           several constraints on one beam: Q_p rows and responses a beam on the beamformer's stream
  synth       deterministic synthetic IF scenes
  build       hipcc build recipe
"""
from . import _lib  # noqa: F401
from ._lib import GmError, lib, library_path  # noqa: F401
from .resample import Resampler  # noqa: F401
from .excise import Excisor  # noqa: F401
from .ddc import Ddc  # noqa: F401
from .channelizer import Channelizer  # noqa: F401
from .nuller import Nuller  # noqa: F401
from .stap import Stap  # noqa: F401
from .beamformer import Beamformer  # noqa: F401
from .lcmv import Lcmv  # noqa: F401
from . import tracking  # noqa: F401
# per-antenna prompts of an array stream at tracked states: TrackingManager.array_prompts, and tracking.array_plan under a name that
# does not collide with acquisition.array_plan
from .tracking import TrackingManager, array_plan as trk_array_plan  # noqa: F401
# tracking on planes: the plane ring a multi-output stage's planes go into, and the two host-only plans
from .tracking import PlaneRing, plane_ring_plan, planes_plan as trk_planes_plan  # noqa: F401
