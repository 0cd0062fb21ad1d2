"""``python -m seamless_communication_amd.audio_to_units <audio> --kmeans_uri ...``: raw audio to units, the counterpart
of the reference's ``m4t_audio_to_units`` (cli/m4t/audio_to_units/audio_to_units.py): same arguments and defaults, the units
are logged as ``Converted to units: tensor([...])``.  HIP devices only; ``kmeans_uri`` must be reachable offline."""
from __future__ import annotations

import argparse
import logging
from typing import Optional, Sequence

import torch

logging.basicConfig(level=logging.INFO)
logger = logging.getLogger(__name__)

DEFAULT_KMEANS_URI = "https://dl.fbaipublicfiles.com/seamlessM4T/models/unit_extraction/kmeans_10k.npy"


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Convert raw audio to units (and optionally audio) using UnitExtractor.")
    parser.add_argument("audio", type=str, help="Audio WAV file path.")
    parser.add_argument("--kmeans_uri", type=str, help="URL path to the K-Means model.", default=DEFAULT_KMEANS_URI)
    parser.add_argument("--model_name", type=str, help="Feature extraction model name (`xlsr2_1b_v2`)", default="xlsr2_1b_v2")
    parser.add_argument("--out_layer_number", type=int, help="Layer number of the feature extraction model to pull out features from.",
                        default=35)
    return parser


def main(argv: Optional[Sequence[str]] = None, extractor_cls=None) -> torch.Tensor:
    args = build_parser().parse_args(argv)
    if extractor_cls is None:
        from .inference import UnitExtractor as extractor_cls
    if not torch.cuda.is_available() and extractor_cls.__module__.startswith("seamless_communication_amd"):
        raise SystemExit("audio_to_units: no HIP device is visible (the UnitExtractor has no CPU path)")
    logger.info("Running unit_extraction on the GPU.")
    unit_extractor = extractor_cls(args.model_name, args.kmeans_uri, device=torch.device("cuda:0"))
    units = unit_extractor.predict(args.audio, args.out_layer_number - 1)
    logger.info(f"Converted to units: {units}")
    return units


if __name__ == "__main__":
    main()
