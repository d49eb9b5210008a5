"""Mirror of `puresound.streaming` (chunked / frame-by-frame forward of the SkiM masker), and hop-by-hop streaming of the
causal conv-STFT U-Net noise suppressors (spectral.py), of the causal time-domain Conv-TasNet (tcn.py) of the causal time-domain DPRNN (dprnn.py),
of the causal time-domain SkiM speaker extractors (skim.py) and of the causal conv-STFT U-Net + gated-TCN speaker extractor
(unet_tcn.py)."""
from .dprnn import StreamingDPRNN  # noqa: F401
from .skim import StreamingSkiMExtractor  # noqa: F401
from .skim_inference import StreamingSkiM  # noqa: F401
from .spectral import StreamingSeparator  # noqa: F401
from .tcn import StreamingConvTasNet  # noqa: F401
from .unet_tcn import StreamingUnetTcn  # noqa: F401
