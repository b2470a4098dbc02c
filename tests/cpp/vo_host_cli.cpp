// Host driver of the VO loop's track table and arithmetic (vo_tracks.hpp, vo_math.hpp; vo_blocks.hpp for the
// tracker's upload size): no HIP, no libme_hip.so.  tests/test_vo_loop_host.py writes the inputs, runs this and
// checks what comes back against feature_types.WBA_Point and pipeline.py.  Floats cross as raw bits.
//
//   vo_host_cli tracks <script.bin> <out.txt>   a script of keyframes through the table, in the loop's step order
//   vo_host_cli math   <in.bin>     <out.bin>   sections of inputs through the arithmetic
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <vector>

#include "../../uasl_motion_estimation_amd/csrc/vo_blocks.hpp"
#include "../../uasl_motion_estimation_amd/csrc/vo_math.hpp"
#include "../../uasl_motion_estimation_amd/csrc/vo_tracks.hpp"

namespace {

using namespace me_vo;

struct Reader {
  std::vector<uint8_t> buf;
  size_t pos = 0;
  bool ok = true;
  explicit Reader(const char* path) {
    if (FILE* f = std::fopen(path, "rb")) {
      uint8_t tmp[4096];
      size_t n;
      while ((n = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
      std::fclose(f);
    } else {
      ok = false;
    }
  }
  bool done() const { return pos >= buf.size(); }
  template <class T>
  T get() {
    T v{};
    if (pos + sizeof(T) > buf.size()) {
      ok = false;
      pos = buf.size();
      return v;
    }
    std::memcpy(&v, &buf[pos], sizeof(T));
    pos += sizeof(T);
    return v;
  }
  template <class T>
  std::vector<T> many(int64_t n) {
    std::vector<T> v;
    for (int64_t i = 0; i < n && ok; ++i) v.push_back(get<T>());
    return v;
  }
};

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
uint64_t bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}

// ---------------------------------------------------------------- tracks
// Script: int32 window, n_frames; per frame mask[8] (k-th active track continues), sub[8] (k-th active track is in
// the second, partial tracker upload), 8 x {u, v, xr} float32 of the tracked slots, int32 n_cand, n_cand x {u, v,
// xr float32, ok uint8}.  The landmark of track id is (id, id + 0.25, id + 0.5): rows are recognisable after a
// compaction.  Output: one record per line, see the prints.
void dump_table(FILE* o, const char* tag, const TrackTable& tab) {
  std::fprintf(o, "%s %d %zu", tag, tab.gen, tab.size());
  for (size_t i = 0; i < tab.size(); ++i)
    std::fprintf(o, " %" PRId64 " %" PRId64 " %" PRId64 " %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64, tab.ids[i],
                 tab.first[i], tab.last[i], (int)tab.active[i], bits(tab.X[3 * i]), bits(tab.X[3 * i + 1]),
                 bits(tab.X[3 * i + 2]));
  std::fprintf(o, "\n");
}
void dump_resolves(FILE* o, int when, const TrackTable& tab, const std::deque<BaRec>& recs) {
  for (const BaRec& r : recs) {
    std::vector<int64_t> j;
    std::vector<uint8_t> live;
    tab.resolve(r, j, live);
    std::fprintf(o, "R %d %d %d %d %zu", when, r.t, r.gen, tab.gen, j.size());
    for (size_t i = 0; i < j.size(); ++i) std::fprintf(o, " %" PRId64 " %" PRId64 " %d", r.wids[i], j[i], (int)live[i]);
    std::fprintf(o, "\n");
  }
}
void dump_upload(FILE* o, int kind, bool same, const TrackTable& tab, const std::vector<int64_t>& rows,
                 const std::vector<float>& pts, const std::vector<float>& pxr) {
  std::fprintf(o, "U %d %d %zu", kind, (int)same, rows.size());
  for (size_t k = 0; k < rows.size(); ++k)
    std::fprintf(o, " %" PRId64 " %08x %08x %08x", tab.ids[rows[k]], bits(pts[2 * k]), bits(pts[2 * k + 1]), bits(pxr[k]));
  std::fprintf(o, "\n");
}

int run_tracks(const char* in, const char* out) {
  Reader r(in);
  FILE* o = std::fopen(out, "w");
  if (!r.ok || !o) return 2;
  const int window = r.get<int32_t>(), n_frames = r.get<int32_t>();
  TrackTable tab;
  tab.log_events = true;
  std::deque<BaRec> recs;
  size_t ev_done = 0;
  for (int t = 0; t <= n_frames && r.ok; ++t) {
    const bool drain = t == n_frames;  // behind the script: everything popped, the table left empty
    std::fprintf(o, "F %d\n", t);
    std::vector<uint8_t> mask(8, 0), sub(8, 0);
    std::vector<float> trk(24, 0.0f), cand;
    std::vector<uint8_t> cand_ok;
    if (!drain) {
      mask = r.many<uint8_t>(8);
      sub = r.many<uint8_t>(8);
      trk = r.many<float>(24);
      const int n_cand = r.get<int32_t>();
      for (int k = 0; k < n_cand; ++k) {
        for (int q = 0; q < 3; ++q) cand.push_back(r.get<float>());
        cand_ok.push_back(r.get<uint8_t>());
      }
      if (!r.ok) break;
    }
    // 1. the tracker's upload: all active rows, then the sub-set of them
    std::vector<int64_t> act;
    tab.active_rows(act);
    if (!drain && t > 0 && !act.empty()) {
      for (int kind = 0; kind < 2; ++kind) {
        std::vector<int64_t> rows;
        for (size_t k = 0; k < act.size(); ++k)
          if (kind == 0 || sub[k]) rows.push_back(act[k]);
        const KltIn kin{rows.size(), false, true};
        std::vector<float> pts(kin.o_guess() / 4), pxr(kin.size() / 4 - pts.size());
        const bool same = rows.empty() ? false : tab.klt_upload(t - 1, rows, pts, pxr);
        dump_upload(o, kind, same, tab, rows, pts, pxr);
      }
    }
    // 2. the pop of frame t - 1's completion
    if (t > 0) {
      std::vector<int> frames;
      std::vector<int64_t> gone;
      const int g0 = tab.gen, new_first = drain ? n_frames + window : t - window;
      tab.pop(new_first, frames, gone);
      std::fprintf(o, "P %d %d %d %zu", new_first, g0, tab.gen, frames.size());
      for (int fr : frames) std::fprintf(o, " %d", fr);
      std::fprintf(o, " %zu", gone.size());
      for (int64_t id : gone) std::fprintf(o, " %" PRId64, id);
      std::fprintf(o, "\n");
    }
    dump_table(o, "T0", tab);
    dump_resolves(o, 0, tab, recs);
    if (!drain) {
      // 4. the tracked features that continue
      tab.active_rows(act);
      std::vector<int64_t> trk_idx;
      std::vector<float> trk_uv, xr_trk;
      for (size_t k = 0; k < act.size(); ++k) {
        if (!mask[k % 8]) {
          tab.active[act[k]] = 0;
          continue;
        }
        trk_idx.push_back(act[k]);
        trk_uv.push_back(trk[3 * (k % 8)]);
        trk_uv.push_back(trk[3 * (k % 8) + 1]);
        xr_trk.push_back(trk[3 * (k % 8) + 2]);
      }
      // 5. the frame booked
      std::vector<float> nuv, nxr;
      std::vector<double> new_X;
      int64_t id = tab.latest_id;
      for (size_t k = 0; k < cand_ok.size(); ++k) {
        nuv.push_back(cand[3 * k]);
        nuv.push_back(cand[3 * k + 1]);
        nxr.push_back(cand[3 * k + 2]);
        if (cand_ok[k]) {
          for (double q : {0.0, 0.25, 0.5}) new_X.push_back((double)id + q);
          ++id;
        }
      }
      std::vector<int64_t> fid, new_ids;
      tab.book(t, trk_idx, trk_uv, xr_trk, nuv, nxr, cand_ok, new_X, fid, new_ids);
      std::fprintf(o, "B %d %zu", t, fid.size());
      for (int64_t i : fid) std::fprintf(o, " %" PRId64, i);
      std::fprintf(o, " %zu", new_ids.size());
      for (int64_t i : new_ids) std::fprintf(o, " %" PRId64, i);
      std::fprintf(o, "\n");
      // 8. the window's rows
      BaRec rec;
      rec.t = t;
      rec.f0 = std::max(0, t - window + 1);
      std::vector<int32_t> wid32;
      std::vector<double> Xw;
      const bool fits = tab.window_rows(rec.f0, rec, wid32, Xw);
      std::fprintf(o, "W %d %d %d %zu", rec.f0, (int)fits, rec.gen, rec.upts.size());
      for (size_t i = 0; i < rec.upts.size(); ++i)
        std::fprintf(o, " %" PRId64 " %" PRId64 " %d %016" PRIx64, rec.upts[i], rec.wids[i], wid32[i], bits(Xw[3 * i]));
      std::fprintf(o, "\n");
      recs.push_back(rec);
      dump_table(o, "T1", tab);
      dump_resolves(o, 1, tab, recs);
      // kf_seed's positions
      std::vector<float> ref, xr;
      tab.seeded(t, true, ref, xr);
      std::fprintf(o, "S %zu", xr.size());
      for (size_t k = 0; k < xr.size(); ++k) std::fprintf(o, " %08x %08x %08x", bits(ref[2 * k]), bits(ref[2 * k + 1]), bits(xr[k]));
      std::fprintf(o, "\n");
    }
    // the observation store, and the events of this frame
    for (const auto& kv : tab.obs) {
      std::fprintf(o, "O %d %zu", kv.first, kv.second.ids.size());
      for (size_t q = 0; q < kv.second.ids.size(); ++q) {
        std::fprintf(o, " %" PRId64, kv.second.ids[q]);
        for (int c = 0; c < 4; ++c) std::fprintf(o, " %08x", bits(kv.second.feats[4 * q + c]));
      }
      std::fprintf(o, "\n");
    }
    for (; ev_done < tab.events.size(); ++ev_done) {
      const me_vo_event& e = tab.events[ev_done];
      std::fprintf(o, "E %d %d %" PRId64 " %08x %08x %08x %08x\n", (int)e.kind, (int)e.t, (int64_t)e.id, bits(e.feat[0]),
                   bits(e.feat[1]), bits(e.feat[2]), bits(e.feat[3]));
    }
  }
  std::fprintf(o, "END %d\n", (int)r.ok);
  std::fclose(o);
  return r.ok ? 0 : 3;
}

// ---------------------------------------------------------------- math
// Sections, each int64 tag and its payload (integers int64, reals float64 unless said otherwise); the results are
// written in order, raw.
template <class T>
void put(FILE* o, const T* p, size_t n) {
  if (n) std::fwrite(p, sizeof(T), n, o);  // (an empty vector's data() may be null)
}

int run_math(const char* in, const char* out) {
  Reader r(in);
  FILE* o = std::fopen(out, "wb");
  if (!r.ok || !o) return 2;
  while (!r.done() && r.ok) {
    const int64_t tag = r.get<int64_t>();
    if (tag == 1) {  // n x aa[3] -> rot_series[9], aa_to_R[9]
      const int64_t n = r.get<int64_t>();
      for (int64_t i = 0; i < n; ++i) {
        const auto aa = r.many<double>(3);
        const Mat3 a = rot_series(aa.data()), b = aa_to_R(aa.data());
        put(o, a.data(), 9);
        put(o, b.data(), 9);
      }
    } else if (tag == 2) {  // n x {X[3], R[9], pose[6], pose2[6], R2[9]} -> X[3]
      const int64_t n = r.get<int64_t>();
      for (int64_t i = 0; i < n; ++i) {
        auto X = r.many<double>(3);
        Mat3 R, R2;
        Pose p, p2;
        for (auto& x : R) x = r.get<double>();
        for (auto& x : p) x = r.get<double>();
        for (auto& x : p2) x = r.get<double>();
        for (auto& x : R2) x = r.get<double>();
        move_landmark(X.data(), R, p, p2, R2);
        put(o, X.data(), 3);
      }
    } else if (tag == 3) {  // n x {t, cell} -> jitter[2]
      const int64_t n = r.get<int64_t>();
      for (int64_t i = 0; i < n; ++i) {
        const int64_t t = r.get<int64_t>(), cell = r.get<int64_t>();
        double j[2];
        cell_jitter((int)t, cell, j);
        put(o, j, 2);
      }
    } else if (tag == 4) {  // n x {width, height, n_feats} -> {nx, ny} int64, {cw, ch}
      const int64_t n = r.get<int64_t>();
      for (int64_t i = 0; i < n; ++i) {
        const int64_t w = r.get<int64_t>(), h = r.get<int64_t>(), nf = r.get<int64_t>();
        const Grid g = make_grid((int)w, (int)h, (int)nf);
        const int64_t nn[2] = {g.nx, g.ny};
        const double cc[2] = {g.cw, g.ch};
        put(o, nn, 2);
        put(o, cc, 2);
      }
    } else if (tag == 5) {  // {t, width, height, n_feats, n_good}, n_good x uv float32[2] -> m int64, m x uv float32[2]
      const int64_t t = r.get<int64_t>(), w = r.get<int64_t>(), h = r.get<int64_t>(), nf = r.get<int64_t>(),
                    ng = r.get<int64_t>();
      const auto uv = r.many<float>(2 * ng);
      std::vector<float> res;
      new_cells_host((int)t, (int)ng, uv.data(), make_grid((int)w, (int)h, (int)nf), (int)nf, res);
      const int64_t m = (int64_t)res.size() / 2;
      put(o, &m, 1);
      put(o, res.data(), res.size());
    } else if (tag == 6) {  // {width, height, n}, n x uv float32[2] -> n bytes
      const int64_t w = r.get<int64_t>(), h = r.get<int64_t>(), n = r.get<int64_t>();
      const auto uv = r.many<float>(2 * n);
      for (int64_t i = 0; i < n && r.ok; ++i) {
        const uint8_t b = in_margin(uv[2 * i], uv[2 * i + 1], (int)w, (int)h);
        put(o, &b, 1);
      }
    } else if (tag == 7) {  // {t, has_velocity, n}, first[6], velocity[6], n x {key int64, pose[6]} -> pose[6]
      const int64_t t = r.get<int64_t>(), hv = r.get<int64_t>(), n = r.get<int64_t>();
      Pose first, vel;
      for (auto& x : first) x = r.get<double>();
      for (auto& x : vel) x = r.get<double>();
      std::map<int, Pose> poses;
      for (int64_t i = 0; i < n; ++i) {
        const int64_t key = r.get<int64_t>();
        Pose p;
        for (auto& x : p) x = r.get<double>();
        poses[(int)key] = p;
      }
      if (!r.ok) break;
      const Pose p = predict_pose(poses, (int)t, first, hv ? vel.data() : nullptr);
      put(o, p.data(), 6);
    } else if (tag == 8) {  // {d_min, d_max, n}, n x d_pred -> n x lo int32, n x dvalid bytes
      const int64_t d_min = r.get<int64_t>(), d_max = r.get<int64_t>(), n = r.get<int64_t>();
      const auto dp = r.many<double>(n);
      std::vector<int32_t> lo(dp.size());
      std::vector<uint8_t> dv(dp.size());
      for (size_t i = 0; i < dp.size(); ++i) search_window(dp[i], (int)d_min, (int)d_max, &lo[i], &dv[i]);
      put(o, lo.data(), lo.size());
      put(o, dv.data(), dv.size());
    } else if (tag == 9) {  // cam[4], pose[6], n, n x {u, v, xr} float32 -> n x X[3]
      const auto c = r.many<double>(4);
      Pose p;
      for (auto& x : p) x = r.get<double>();
      const int64_t n = r.get<int64_t>();
      const auto f = r.many<float>(3 * n);
      if (!r.ok) break;
      const Camera cam{c[0], c[1], c[2], c[3]};
      const Mat3 R = aa_to_R(&p[3]);
      for (int64_t i = 0; i < n; ++i) {
        double X[3];
        triangulate(f[3 * i], f[3 * i + 1], f[3 * i + 2], cam, p, R, X);
        put(o, X, 3);
      }
    } else if (tag == 10) {  // cam[4], pose[6], n, n x X[3] -> n x uv float32[2], n x d_pred
      const auto c = r.many<double>(4);
      Pose p;
      for (auto& x : p) x = r.get<double>();
      const int64_t n = r.get<int64_t>();
      const auto X = r.many<double>(3 * n);
      if (!r.ok) break;
      const Camera cam{c[0], c[1], c[2], c[3]};
      const Mat3 R = aa_to_R(&p[3]);
      std::vector<float> uv(2 * (size_t)n);
      std::vector<double> d((size_t)n);
      for (int64_t i = 0; i < n; ++i) {
        predict_uv(&X[3 * i], R, p, cam, &uv[2 * i]);
        d[i] = predicted_disparity(&X[3 * i], R, p, cam);
      }
      put(o, uv.data(), uv.size());
      put(o, d.data(), d.size());
    } else {
      r.ok = false;
    }
  }
  std::fclose(o);
  return r.ok ? 0 : 3;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "tracks") return run_tracks(argv[2], argv[3]);
  if (argc == 4 && std::string(argv[1]) == "math") return run_math(argv[2], argv[3]);
  std::fprintf(stderr, "usage: vo_host_cli tracks|math <in> <out>\n");
  return 1;
}
