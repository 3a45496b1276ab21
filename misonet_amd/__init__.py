"""misonet_amd -- MI355X-native MISO1 -> MVDR -> MISO3 inference path (hand-written HIP behind a C ABI).

Host-side mirror of the reference call surface:
  MISO_1, MISO_3            (reference model.py:8-111, 282-395)
  Apply_Beamforming         (reference tester.py:1071-1136)
  Beamformer                (the options of the selectable beamformers: mvdr / souden / gev, MPDR, conditioning, BAN; and
                             of the WPD convolutional beamformer, kind "wpd")
  Apply_Beamforming_Joint   (the joint multi-speaker beamformers: LCMV, SDW-MWF, rank-1 MWF; JointBeamformer: their options)
  dereverb, dereverb_wav    (WPE dereverberation of spectrograms / of a whole recording; Dereverb: its options)
  DereverbStream, dereverb_online  (online WPE: the frame-recursive form, fed audio as it arrives, its state carried from call
                             to call; OnlineDereverb: its options)
  cacgmm, masks_from_estimates  (guided spatial clustering between MISO1 and the beamformer; Refine: its options)
  auxiva, BlindSeparator    (blind separation, AuxIVA-ISS: a front end that needs no weights; AuxIVA: its options)
  SeparateStream, auxiva_online   (online AuxIVA: frame-recursive separation, state carried; OnlineAuxIVA: its options; with
                             num_src = K below the number of microphones the overdetermined form: K rows out)
  BeamformStream, beamform_online  (online beamformer: frame-recursive Souden MVDR / rank-1 MWF behind the online separation,
                             state carried; OnlineBeamformer: its options)
  StftStream, IstftStream   (streaming STFT / iSTFT: waveform blocks in, frames out; frames in, waveform blocks out; the bits
                             of the offline kernels however the stream is cut)
  StreamSeparator, separate_stream  (the causal chain from waveform block to waveform block: StftStream -> online WPE ->
                             online AuxIVA -> online beamformer -> IstftStream, misonet_amd.stream)
  resample, resampled_len, load_wav  (recordings at any sample rate: the polyphase resampler of scipy.signal.resample_poly's
                             definition, in front of and behind every recording path)
  ResampleStream            (the same resampler fed in blocks, state carried: the bits of resample however the stream is cut;
                             the two ends of StreamSeparator at any rate)
  Room, simulate, beta_from_rt60  (room simulator: image-source RIRs of a shoebox and scene mixing, misonet_amd.room; Scene:
                             what simulate returns)
  Localizer, localize, localize_wav, DoaResult  (source localisation: SRP, SRP-PHAT and MUSIC maps over a delay table and their
                             peaks, misonet_amd.localize; directions, far_field_delays, near_field_delays, angular_error: its
                             host helpers)
  Enhancer                  (reference tester.py:846-975, the Tester_Enhance hot loop, kept on-device)
  tester.Tester_Enhance     (reference tester.py:798-975: the harness class itself, same constructor / test / inference)
The compute lives in csrc/ (libmisonet_hip.so); importing a compute symbol without the built
library raises -- there is no CPU fallback.
"""
__all__ = ["MISO_1", "MISO_3", "Apply_Beamforming", "Beamformer", "Apply_Beamforming_Joint", "JointBeamformer", "Dereverb", "dereverb", "dereverb_wav", "Refine", "cacgmm",
           "OnlineDereverb", "DereverbStream", "dereverb_online",
           "masks_from_estimates", "AuxIVA", "auxiva", "BlindSeparator", "OnlineAuxIVA", "SeparateStream", "auxiva_online",
           "OnlineBeamformer", "BeamformStream", "beamform_online", "StftStream", "IstftStream", "StreamSeparator",
           "separate_stream", "resample", "resampled_len", "ResampleStream",
           "load_wav", "Room", "Scene", "simulate", "beta_from_rt60", "Localizer", "localize", "localize_wav",
           "DoaResult", "directions", "far_field_delays", "near_field_delays", "angular_error", "Enhancer", "weights"]


def __getattr__(name):
    if name in ("MISO_1", "MISO_3"):
        from . import model
        return getattr(model, name)
    if name == "Apply_Beamforming":
        from .beamform import Apply_Beamforming
        return Apply_Beamforming
    if name == "Beamformer":
        from .beamform import Beamformer
        return Beamformer
    if name in ("Apply_Beamforming_Joint", "JointBeamformer", "OnlineBeamformer", "BeamformStream", "beamform_online"):
        from . import beamform
        return getattr(beamform, name)
    if name in ("Dereverb", "dereverb", "dereverb_wav", "OnlineDereverb", "DereverbStream", "dereverb_online"):
        import importlib
        return getattr(importlib.import_module(".dereverb", __name__), name)
    if name in ("Refine", "cacgmm", "masks_from_estimates"):
        import importlib
        return getattr(importlib.import_module(".refine", __name__), name)
    if name in ("AuxIVA", "auxiva", "BlindSeparator", "OnlineAuxIVA", "SeparateStream", "auxiva_online"):
        import importlib
        return getattr(importlib.import_module(".blind", __name__), name)
    if name in ("StftStream", "IstftStream"):
        import importlib
        return getattr(importlib.import_module(".stft", __name__), name)
    if name in ("StreamSeparator", "separate_stream"):
        import importlib
        return getattr(importlib.import_module(".stream", __name__), name)
    if name in ("resample", "resampled_len", "load_wav", "ResampleStream"):
        import importlib
        return getattr(importlib.import_module(".resample", __name__), name)
    if name in ("Room", "Scene", "simulate", "beta_from_rt60"):
        import importlib
        return getattr(importlib.import_module(".room", __name__), name)
    if name in ("Localizer", "localize", "localize_wav", "DoaResult", "directions", "far_field_delays", "near_field_delays",
                "angular_error"):
        import importlib
        return getattr(importlib.import_module(".localize", __name__), name)
    if name == "Enhancer":
        from .pipeline import Enhancer
        return Enhancer
    if name == "weights":
        import importlib
        return importlib.import_module(".weights", __name__)
    raise AttributeError(name)
