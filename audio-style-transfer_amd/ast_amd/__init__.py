"""ast_amd -- MI355X-native (gfx950) hot path of francescobrigante/Audio-Style-Transfer.

Drop-in modules keep the reference's call surface (StyleEncoder, ContentEncoder,
Decoder, Discriminator, losses, utilityFunctions); all arithmetic runs in
hand-written HIP kernels behind the C-ABI of include/ast_hip.h.  There is no CPU
or ATen fallback: without libast_hip.so and a GPU the ops raise.
"""
from . import config  # noqa: F401
from .config import set_compute_dtype, set_deterministic  # noqa: F401
from .style_encoder import StyleEncoder, SinusoidalPositionalEncoding, initialize_weights  # noqa: F401
from .content_encoder import ContentEncoder  # noqa: F401
from .new_decoder import Decoder, compute_comprehensive_loss  # noqa: F401
from .discriminator import Discriminator  # noqa: F401
from .losses import infoNCE_loss, margin_loss, adversarial_loss, disentanglement_loss, reconstruction_losses  # noqa: F401
from .losses import ragged_reconstruction_loss  # noqa: F401
from .metrics import mse_spectrogram, band_energy, instrumentation_similarity, mfcc, mfcc_distance  # noqa: F401
from .metrics import estimate_tuning, chroma_stft, chroma_distance, chroma_similarity, pitch_mean, pitch_correlation  # noqa: F401
from .metrics import onset_strength, onset_detect, onset_accuracy, recurrence_matrix, self_similarity_distance  # noqa: F401
from .curation import frame_rms, silence_ratio, clip_rms, sound_windows, sound_ratio, mfcc_mean, rms_normalize, screen, DatasetReport  # noqa: F401


class deterministic:
    """Context manager: deterministic mode inside the block (config.set_deterministic), the previous setting restored after it.
    `with ast_amd.deterministic(): ...`  /  `with ast_amd.deterministic(False): ...`"""

    def __init__(self, flag=True):
        self.flag = bool(flag)

    def __enter__(self):
        self.prev = config.deterministic
        config.set_deterministic(self.flag)
        return self

    def __exit__(self, *exc):
        config.deterministic = self.prev
        return False
