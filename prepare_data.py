"""Recordings + alignments -> the trainer's dataset (reference: prepare_data.py): reads ./config.yaml and runs
`Preprocessor(preprocess_config).build_from_path()` over `path.raw_path` into `path.preprocessed_path` (tts_king_amd/preprocess.py).
With `mi355x.align_missing: true` an utterance without a `.TextGrid` is aligned on the device with the model at `tts.weights_path`
(tts_king_amd/align.py) instead of being skipped."""
from tts_king_amd.config import load_config
from tts_king_amd.preprocess import Preprocessor


def build_aligner(cfg):
    """The `Aligner` of `mi355x.align_missing: true` (None without the key), on the model `tts.weights_path` names."""
    mi = cfg.get("mi355x", {}) or {}
    if not mi.get("align_missing", False):
        return None
    import copy
    from fsapi import FSTWOapi
    from tts_king_amd.align import Aligner
    if cfg.tts.weights_path is None:
        raise ValueError("mi355x.align_missing: true needs a model to align with: set tts.weights_path")
    model_cfg = copy.deepcopy(cfg)          # FSTWOapi points its copy's preprocessed_path at the checkpoint's folder; the output path stays
    tts = FSTWOapi(model_cfg, cfg.gpu)
    return Aligner(tts, cfg.preprocess_config, tts.device)


if __name__ == "__main__":
    cfg = load_config("./config.yaml")
    mi = cfg.get("mi355x", {}) or {}
    preprocessor = Preprocessor(cfg.preprocess_config, use_cwt=bool(cfg.model_config.get("use_cwt", False)), aligner=build_aligner(cfg),
                                align_max_cost=mi.get("align_max_cost"), new_speaker_init=mi.get("new_speaker_init"))
    out = preprocessor.build_from_path()
    print("%d utterances, %.3f hours; left out: %s" % (len(out), preprocessor.hours, preprocessor.skipped))
