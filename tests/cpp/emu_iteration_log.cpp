// TEST INFRASTRUCTURE — the emulated pipeline (emu_pipeline.cpp, included as it stands) with an entry that records the iteration
// log (include/limo_hip.h:limo_ba_iteration): the same lm_* / sched_* functions the kernels call write the entries, the emulator only
// hands every window its buffer.  Built by tests/iteration_log_common.py into tests/cpp/_build/libkba_emu_itlog.so.
#include "emu_pipeline.cpp"

extern "C" {

// n_slots > 0: the streaming schedule with that many windows in flight, else the lock-step schedule.  lm_fixed: NULL, or per window
// NULL or its constness flags.  Window w records into log[w * cap .. w * cap + cap); log_n[w] = the entries it has.
int emu_ba_solve_batch_log(int32_t n, limo_ba_window* windows, const uint8_t* const* lm_fixed, const limo_ba_options* o, limo_ba_report* reports,
                           int pose_only, const limo_speed_prior* prior, int n_slots, int32_t cap, limo_ba_iteration* log, int32_t* log_n) {
    EmuBatch B;
    std::string err;
    PackOptions po;
    po.pose_only = pose_only != 0;
    po.prior = prior;
    po.lm_fixed = lm_fixed;
    int rc = pack_windows(n, windows, *o, po, B.P, err);
    if (rc != LIMO_OK) return rc;
    B.c = make_consts(*o);
    B.alloc();
    for (int w = 0; w < n; ++w) {
        B.bv.st[w].log = log + (size_t)w * cap;
        B.bv.st[w].log_cap = cap;
    }
    if (n_slots > 0)
        B.run_streaming(n_slots);
    else
        run_schedule(B, *o);
    write_back(B, windows);
    record_trimmed(B);
    for (int w = 0; w < n; ++w) {
        log_n[w] = B.bv.st[w].log_n;
        if (reports) fill_report(B, w, reports + w);
    }
    return LIMO_OK;
}

int emu_iteration_size(void) { return (int)sizeof(limo_ba_iteration); }

}  // extern "C"
