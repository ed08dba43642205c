from .checkpoint import load_checkpoint, save_checkpoint, str_to_bool
from .trainer import Trainer, strong_loss, weak_loss

__all__ = ["load_checkpoint", "save_checkpoint", "str_to_bool", "Trainer", "strong_loss", "weak_loss"]
