from .collator import VLDPODataCollatorWithPadding, VLKTODataCollatorWithPadding  # noqa: F401
from .processor import VLChatTemplate, VLProcessor  # noqa: F401
from .trainer import KTOConfig, VLDPOTrainer, VLKTOTrainer  # noqa: F401
