"""Recordings + alignments -> the trainer's dataset (reference: prepare_data.py): reads ./config.yaml and runs
`Preprocessor(preprocess_config).build_from_path()` over `path.raw_path` into `path.preprocessed_path` (tts_king_amd/preprocess.py)."""
from tts_king_amd.config import load_config
from tts_king_amd.preprocess import Preprocessor


if __name__ == "__main__":
    cfg = load_config("./config.yaml")
    preprocessor = Preprocessor(cfg.preprocess_config, use_cwt=bool(cfg.model_config.get("use_cwt", False)))
    out = preprocessor.build_from_path()
    print("%d utterances, %.3f hours; left out: %s" % (len(out), preprocessor.hours, preprocessor.skipped))
