"""The entry points tests/test_gpu_caller_stream.py runs on a caller's own stream, by what each does to that stream.  Data
only: tests/test_world_arguments_host.py holds the three sets below to WorldBatch's public methods without a device."""

# Which entry points return without a host round trip once their one-off set-ups are made (the warm-up): for these the
# delay must still be running when the call returns.  Read from the code, not tried.
ASYNC = ("dio", "harvest", "stonemask", "cheaptrick", "d4c", "analyze", "samples_from_pcm16", "samples_to_pcm16",
         "utterance_status", "code_spectral_envelope", "decode_spectral_envelope", "code_aperiodicity",
         "decode_aperiodicity", "recipe_features", "recipe_decode", "compose_cmp", "compose_ffo", "interpolate_gaps",
         "column_moments", "utterance_means", "mel_cepstrum", "spectrum_from_mel_cepstrum", "postfilter_mel_cepstrum",
         "modulation_spectrum_stats", "postfilter_modulation_spectrum", "parameter_generation", "trajectory_cost",
         "acoustic_model_forward", "acoustic_model_train_forward", "acoustic_model_backward",
         "dtw_align", "feature_distortion", "mlsa_synthesis", "parameter_generation_gv",
         "convert_mel_generalized_cepstrum", "modify_features",
         # mlsa.hip, launch_mlsa_excitation and launch_mlsa_filter: the noise table and the workspace are one-off (grow_ws),
         # the taps travel as kernel arguments (upload_taps), the Pade row is host arithmetic; the rest is launches
         "mlsa_excitation", "mlsa_filter",
         # mgcep.hip: launch_mgcep is one launch; the waveform form's window goes up by hipMemcpyAsync from the batch's own
         # h_win, pageable, which returns once the source is staged (as dnn.hip's h_spk does in acoustic_model_forward)
         "mel_cepstrum_of_frames", "mel_cepstrum_of_waveform",
         "optimizer_step")
# ... and the ones that wait for the stream inside, each with the line that does
SYNCHRONISES = {
    "synthesize": "synthesis.hip, synthesis_prepare_wait: hipStreamSynchronize(st) -- the pulse count read on the host "
                  "sizes the response scratch (the split form waits once per part)",
    "analyze_synthesize": "the same round trip of Synthesis's preparation, on the side stream forked from the caller's "
                          "(cold: on the caller's stream itself)",
    "vibrato": "vibrato.hip, launch_vibrato's last step: hipStreamSynchronize(st) -- the uploaded segment arrays are "
               "call-local and *n_too_long is returned to the host",
    "label_features": "ffi.hip, launch_label_features: hipStreamSynchronize(st) on every call of a batch but its first "
                      "-- the upload image and the device block of the call before are reused",
}
COVERED = ASYNC[:-1] + tuple(SYNCHRONISES)          # WorldBatch methods; optimizer_step is the context's
# ... and the public names of WorldBatch that queue nothing
NO_DEVICE_WORK = {"set_f0_estimator", "split_frames", "split_out", "close"}
