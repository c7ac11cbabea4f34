// debug.inc -- the ratsdf_debug_* readers: stamps and counters that the kernels of the diagnostic build (make stamps,
// -DRATSDF_STAMPS) leave in Ctl, printed or copied out.  Included at the end of ratsdf_engine.hip.  (The shipped library
// exports them too, apart from the switch: there they find nothing recorded.)

extern "C" {

// diagnostic: per-wave stamps of the LAST k_integrate launch (stamps build only)
int ratsdf_debug_wave_stamps(ratsdf_engine* e, int enable) {
  ENTRY(e, true);
  // (one buffer per PROCESS, deliberately never freed and so without an owner: an engine's Ctl::debug_buf keeps
  // pointing at it, and a static owner's destructor would call into a HIP runtime that is already shutting down)
  static unsigned long long* buf = nullptr;
  const size_t n = 16384 * 8;
  if (enable > 0) {
    if (!buf) HIPCHK(hipMalloc(&buf, n * 8));
    HIPCHK(hipMemsetAsync(buf, 0, n * 8, e->stream));
    HIPCHK(hipMemcpyAsync(&e->ctl->debug_buf, &buf, sizeof(buf), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RATSDF_OK;
  }
  std::vector<unsigned long long> h(n);
  HIPCHK(hipMemcpyAsync(h.data(), buf, n * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  // k_integrate keeps one half of the buffer per frame parity (the last two frames of a batch stay apart):
  // enable = -1 / -2 reports the half of parity 0 / 1 alone
  if (enable < 0) {
    const size_t keep = (size_t)(-enable - 1);
    for (size_t w = 0; w < 16384; ++w)
      if ((w >> 13) != keep)
        for (int k = 0; k < 8; ++k) h[w * 8 + k] = 0;
  }
  unsigned long long t0 = ~0ull, t1 = 0;
  double ph[4] = {0, 0, 0, 0};
  size_t cnt = 0;
  std::vector<unsigned long long> starts, ends;
  for (size_t w = 0; w < 16384; ++w) {
    const unsigned long long* s = &h[w * 8];
    if (!s[0] || !s[4] || !s[1]) continue;
    t0 = s[5] < t0 ? s[5] : t0;
    t1 = s[6] > t1 ? s[6] : t1;
    ph[0] += (double)(s[1] - s[0]);
    ph[1] += (double)(s[2] - s[1]);
    ph[2] += (double)(s[3] - s[2]);
    ph[3] += (double)(s[4] - s[3]);
    starts.push_back(s[5]);
    ends.push_back(s[6]);
    ++cnt;
  }
  if (!cnt) { fprintf(stderr, "[wave stamps] none\n"); return RATSDF_OK; }
  {  // phase profile of the slowest 5 % of the waves
    std::vector<std::pair<unsigned long long, size_t>> dur;
    for (size_t w = 0; w < 16384; ++w) {
      const unsigned long long* s = &h[w * 8];
      if (!s[0] || !s[4] || !s[1]) continue;
      dur.emplace_back(s[4] - s[0], w);
    }
    std::sort(dur.begin(), dur.end());
    const size_t lo = dur.size() * 95 / 100;
    double q[4] = {0, 0, 0, 0};
    for (size_t i = lo; i < dur.size(); ++i) {
      const unsigned long long* s = &h[dur[i].second * 8];
      q[0] += (double)(s[1] - s[0]); q[1] += (double)(s[2] - s[1]);
      q[2] += (double)(s[3] - s[2]); q[3] += (double)(s[4] - s[3]);
    }
    const double m = (double)(dur.size() - lo);
    fprintf(stderr, "[wave stamps] wave duration cycles: p50 %llu p95 %llu max %llu; slowest 5%% phases: %.0f | %.0f | %.0f | %.0f\n",
            dur[dur.size() / 2].first, dur[lo].first, dur.back().first, q[0] / m, q[1] / m, q[2] / m, q[3] / m);
  }
  std::sort(starts.begin(), starts.end());
  std::sort(ends.begin(), ends.end());
  fprintf(stderr, "[wave stamps] %zu waves (first block of each); span first-start..last-end = %llu ticks of 10 ns\n", cnt, t1 - t0);
  fprintf(stderr, "[wave stamps] mean cycles per phase: %.0f | %.0f | %.0f | %.0f  (k_integrate: issue+project | wait loads | math | store; k_front pixels with RATSDF_DEBUG=8: load+texel | ray math | wait lookups | evaluate)\n",
          ph[0] / cnt, ph[1] / cnt, ph[2] / cnt, ph[3] / cnt);
  fprintf(stderr, "[wave stamps] start spread: p50 %llu p99 %llu max %llu ; end: p1 %llu p50 %llu (relative to first start)\n",
          starts[cnt / 2] - t0, starts[cnt * 99 / 100] - t0, starts[cnt - 1] - t0, ends[cnt / 100] - t0, ends[cnt / 2] - t0);
  {  // the whole launch: when the serial role published, when the waves' LAST passes ended
    unsigned long long st[6], last = 0;
    std::vector<unsigned long long> done;
    for (size_t w = 0; w < 16384; ++w)
      if (h[w * 8 + 7]) done.push_back(h[w * 8 + 7]);
    HIPCHK(hipMemcpyAsync(st, e->ctl->stamps, sizeof(st), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (!done.empty()) {
      std::sort(done.begin(), done.end());
      last = done.back();
      for (int par = 0; par < 2; ++par)
        if ((enable == 0 || par == -enable - 1) && st[par * 3 + 1] > t0 && st[par * 3 + 1] < last)
          fprintf(stderr, "[wave stamps] serial role: started %lld, published at %lld; waves' last passes end: p50 %llu p99 %llu max %llu (10 ns ticks after the first update wave started)\n",
                  (long long)(st[par * 3] - t0), (long long)(st[par * 3 + 1] - t0), done[done.size() / 2] - t0,
                  done[done.size() * 99 / 100] - t0, last - t0);
    }
  }
  return RATSDF_OK;
}

#ifdef RATSDF_STAMPS
// diagnostic (stamps build only): the ablation / fault-injection switch of an engine after its creation (RATSDF_DEBUG
// sets it at creation): tests/test_gpu_errors.py injects a fault, switches it off and recovers
int ratsdf_debug_set_switch(ratsdf_engine* e, int value) {
  if (!e) return RATSDF_ERR_BAD_ARGUMENT;
  e->debug = value;
  return RATSDF_OK;
}
#endif

// diagnostic (stamps build only): the raw per-wave record buffer ratsdf_debug_wave_stamps(e, 1) attached (16 384 x 8
// words), copied out and zeroed -- k_raycast's per-wave timeline (tools/raycast_probe.py)
int ratsdf_debug_wave_records(ratsdf_engine* e, unsigned long long* out, size_t words) {
  ENTRY(e, out && words <= 16384 * 8);
  unsigned long long* buf = nullptr;
  HIPCHK(hipMemcpyAsync(&buf, &e->ctl->debug_buf, sizeof(buf), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (!buf) return RATSDF_ERR_BAD_ARGUMENT;
  HIPCHK(hipMemcpyAsync(out, buf, words * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return RATSDF_OK;
}

// diagnostic (stamps build only): Ctl::dbg -- RATSDF_DEBUG=30 counts update waves that changed no voxel:
// [0] such waves, [1] waves, [2] blocks without an update, [3] blocks; read and reset
int ratsdf_debug_counters(ratsdf_engine* e, unsigned long long* out8) {
  ENTRY(e, out8);
  HIPCHK(hipMemcpyAsync(out8, e->ctl->dbg, 8 * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemsetAsync(e->ctl->dbg, 0, 8 * 8, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return RATSDF_OK;
}

// diagnostic: timeline of k_front's tail (stamps build only): sums over frames of wall-clock ticks (10 ns)
// since the launch's first workgroup started
int ratsdf_debug_tail_stamps(ratsdf_engine* e) {
  ENTRY(e, true);
  unsigned long long t[16];
  HIPCHK(hipMemcpyAsync(t, e->ctl->tstamps, sizeof(t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemsetAsync(e->ctl->tstamps, 0, sizeof(t), e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const double n = t[8] ? (double)t[8] : 1.0;
  fprintf(stderr, "[tail stamps] %llu tail frames; us after the launch's first workgroup started: last directory workgroup "
          "done %.2f | its stores drained %.2f | it knows it is last %.2f | tail: first round of loads in %.2f | claims + "
          "winners listed %.2f | commits issued %.2f | end %.2f ; requests %.1f winners %.1f per frame\n",
          t[8], t[1] / n / 100, t[2] / n / 100, t[3] / n / 100, t[4] / n / 100, t[5] / n / 100, t[6] / n / 100,
          t[7] / n / 100, t[9] / n, t[10] / n);
  if (t[15]) {
    const double m = (double)t[15];
    unsigned long long c[32];
    HIPCHK(hipMemcpyAsync(c, e->ctl->stamps, sizeof(c), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const double k = c[17] ? (double)c[17] : 1.0;
    fprintf(stderr, "[cand stamps] %llu candidate workgroups sampled (wave 0), shader cycles: inputs arrive %.0f | ray set-up %.0f | "
            "sample loop %.0f (%.2f iterations) ; workgroup: set init + barrier %.0f | pixel work %.0f | barrier wait %.0f | "
            "compaction + stores %.0f\n",
            t[15], t[11] / m, t[12] / m, t[13] / m, t[14] / m, c[14] / k, c[15] / k, c[16] / k, c[18] / k);
  }
  return RATSDF_OK;
}

// diagnostic: prints the accumulated phase stamps of the single-workgroup kernels (stamps build only)
int ratsdf_debug_stamps(ratsdf_engine* e) {
  ENTRY(e, true);
  unsigned long long t[32];
  unsigned long long tot[5];
  HIPCHK(hipMemcpyAsync(t, e->ctl->stamps, sizeof(t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(tot, e->ctl->totals, sizeof(tot), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const double n = tot[0] ? (double)tot[0] : 1.0;
  fprintf(stderr, "[stamps] frames=%llu  serial role (shader cycles/frame): loads:%.0f claims+barrier:%.0f lists:%.0f ranks:%.0f tail:%.0f | deletes %.1f winners %.1f requests %.1f per frame\n",
          tot[0], (double)(t[9] - t[8]) / n, (double)(t[10] - t[9]) / n, (double)(t[11] - t[10]) / n,
          (double)(t[12] - t[11]) / n, (double)(t[13] - t[12]) / n, (double)t[16] / n, (double)t[17] / n,
          (double)t[18] / n);
  if (t[29])
    fprintf(stderr, "[stamps] chained-bucket resolver, %llu passes (shader cycles/pass): order + duplicates %.0f | plans %.0f | replay %.0f | apply %.0f | per pass: requests %.1f distinct %.1f stale plans %.2f placed %.1f | step loop %.0f cycles for %.1f steps\n",
            t[29], (double)(t[22] - t[20]) / t[29], (double)(t[23] - t[22]) / t[29], (double)(t[24] - t[23]) / t[29],
            (double)(t[21] - t[24]) / t[29], (double)t[25] / t[29], (double)t[26] / t[29], (double)t[27] / t[29],
            (double)t[28] / t[29], (double)(long long)t[30] / t[29], (double)t[31] / t[29]);
  fprintf(stderr, "[stamps] ranks phase, first pass (cold code) %.0f cycles of the two\n", (double)t[19] / n);
  {
    const double m = t[17] ? (double)t[17] : 1.0;
    fprintf(stderr, "[stamps] candidate pass, thread 0 of sampled workgroups (shader cycles): first barrier %.0f | pixel work %.0f | wait for the workgroup %.0f | compaction + stores %.0f\n",
            (double)t[14] / m, (double)t[15] / m, (double)t[16] / m, (double)t[18] / m);
  }
  return RATSDF_OK;
}

}  // extern "C"
