// vo_tracks.hpp -- the VO loop's track table: the WBA_Point bookkeeping as a structure of arrays (vo_loop.cpp).
//
// include/MotionEstimation/core/feature_types.h:121-197 in table form: IDs from the value constructor's counter
// (latestID++, :137-139), addMatch of contiguous frames (:140), pop() of the oldest feature (:142), empty tracks
// deleted; the BA window in initialiseObservations order (BundleAdjuster.h:354-376).  A row's index is its creation
// order, so the ID column ascends.  The table owns the rows, the per-frame observation store and the event log; it
// knows no device pointer and no context, and nothing of the device window's frame map or the covariance maps:
// pop() returns what left and the loop erases its own entries.  tests/cpp/vo_host_cli.cpp drives it on the CPU
// (tests/test_vo_loop_host.py replays its events through feature_types.WBA_Point).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../include/me_hip.h"

namespace me_vo {

struct FrameObs {
  std::vector<int64_t> ids;  // ascending
  std::vector<float> feats;  // 4 per feature {xl, yl, xr, yr}
};

// A submitted BA window: its frames, its points' IDs and rows at submit time, and the table's generation then
struct BaRec {
  int t = -1, f0 = 0;
  std::vector<int64_t> wids, upts;
  int nobs = 0, gen = 0;
};

struct TrackTable {
  std::vector<int64_t> ids, first, last;  // first: the oldest frame still held (after pops)
  std::vector<double> X;                  // 3 per track
  std::vector<uint8_t> active;
  int64_t latest_id = 0;
  int gen = 0;                  // compactions so far
  std::vector<int64_t> remap;   // the last compaction's index map (-1: deleted)
  std::map<int, FrameObs> obs;  // frame -> its features
  bool log_events = false;
  std::vector<me_vo_event> events;  // kind 0 new, 1 add, 2 pop, 3 del

  size_t size() const { return ids.size(); }
  int64_t find_id(int64_t id) const {  // searchsorted in the ascending ID column
    return std::lower_bound(ids.begin(), ids.end(), id) - ids.begin();
  }
  void active_rows(std::vector<int64_t>& act) const {
    act.clear();
    for (size_t i = 0; i < size(); ++i)
      if (active[i]) act.push_back((int64_t)i);
  }

  // Step 1, the tracker's upload: the rows' positions in frame prev_t, and their x_r there for the gate (pxr
  // sized by the caller: empty without the gate).  Returns whether the rows are exactly prev_t's features in order
  // (then no search is needed); otherwise each is found by its ID.
  bool klt_upload(int prev_t, const std::vector<int64_t>& act, std::vector<float>& pts, std::vector<float>& pxr) const {
    const FrameObs& po = obs.at(prev_t);
    const bool same = po.ids.size() == act.size() &&
                      std::equal(act.begin(), act.end(), po.ids.begin(), [&](int64_t a, int64_t pid) { return ids[a] == pid; });
    for (size_t k = 0; k < act.size(); ++k) {
      const size_t pos =
          same ? k : (size_t)(std::lower_bound(po.ids.begin(), po.ids.end(), ids[act[k]]) - po.ids.begin());
      pts[2 * k] = po.feats[4 * pos];
      pts[2 * k + 1] = po.feats[4 * pos + 1];
      if (!pxr.empty()) pxr[k] = po.feats[4 * pos + 2];
    }
    return same;
  }

  // Step 5, frame t booked: the accepted new features (nok) become tracks with the next IDs and the landmarks
  // new_X (3 per accepted feature, in order); the tracked rows trk_idx and the new rows are merged by table index
  // (= ID order; stable), `last`, the frame's observations and the new / add events written.  fid: the frame's
  // IDs, ascending; new_ids: the new tracks'.
  void book(int t, const std::vector<int64_t>& trk_idx, const std::vector<float>& trk_uv, const std::vector<float>& xr_trk,
            const std::vector<float>& nuv, const std::vector<float>& nxr, const std::vector<uint8_t>& nok,
            const std::vector<double>& new_X, std::vector<int64_t>& fid, std::vector<int64_t>& new_ids) {
    std::vector<int64_t> new_idx;
    std::vector<float> new_feats;
    const size_t n0 = size();
    for (size_t k = 0; k < nok.size(); ++k) {
      if (!nok[k]) continue;
      const double* Xn = &new_X[3 * new_idx.size()];
      ids.push_back(latest_id++);
      X.insert(X.end(), Xn, Xn + 3);
      active.push_back(1);
      first.push_back(t);
      last.push_back(t);
      new_idx.push_back((int64_t)(n0 + new_feats.size() / 4));
      new_feats.insert(new_feats.end(), {nuv[2 * k], nuv[2 * k + 1], nxr[k], nuv[2 * k + 1]});
    }
    // tracked first, then new; sorted by table index (= ID order; stable)
    const size_t nf = trk_idx.size() + new_idx.size();
    std::vector<int64_t> idx(nf);
    std::vector<uint8_t> is_new(nf, 0);
    FrameObs fo;
    fo.feats.resize(4 * nf);
    {
      std::vector<std::pair<int64_t, size_t>> ord(nf);
      for (size_t k = 0; k < trk_idx.size(); ++k) ord[k] = {trk_idx[k], k};
      for (size_t k = 0; k < new_idx.size(); ++k) ord[trk_idx.size() + k] = {new_idx[k], trk_idx.size() + k};
      std::stable_sort(ord.begin(), ord.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
      for (size_t q = 0; q < nf; ++q) {
        const size_t k = ord[q].second;
        idx[q] = ord[q].first;
        if (k < trk_idx.size()) {
          const float fe[4] = {trk_uv[2 * k], trk_uv[2 * k + 1], xr_trk[k], trk_uv[2 * k + 1]};
          std::memcpy(&fo.feats[4 * q], fe, 16);
        } else {
          std::memcpy(&fo.feats[4 * q], &new_feats[4 * (k - trk_idx.size())], 16);
          is_new[q] = 1;
        }
      }
    }
    fo.ids.resize(nf);
    for (size_t q = 0; q < nf; ++q) {
      fo.ids[q] = ids[idx[q]];
      last[idx[q]] = t;
    }
    if (log_events)
      for (size_t q = 0; q < nf; ++q) {
        me_vo_event e{is_new[q] ? 0 : 1, t, fo.ids[q], {0, 0, 0, 0}};
        std::memcpy(e.feat, &fo.feats[4 * q], 16);
        events.push_back(e);
      }
    new_ids.resize(new_idx.size());
    for (size_t k = 0; k < new_idx.size(); ++k) new_ids[k] = ids[new_idx[k]];
    fid = fo.ids;
    obs[t] = std::move(fo);
  }

  // Frames older than new_first leave the store (every feature of theirs popped; a track that lives on has its
  // `first` bumped), then the tracks last seen before new_first are deleted and the table compacted (gen + 1,
  // remap).  Nothing to delete: the rows, gen and remap stay as they are.
  void pop(int new_first, std::vector<int>& popped_frames, std::vector<int64_t>& deleted_ids) {
    popped_frames.clear();
    deleted_ids.clear();
    while (!obs.empty() && obs.begin()->first < new_first) {
      auto it = obs.begin();
      const int fr = it->first;
      if (log_events)
        for (int64_t id : it->second.ids) events.push_back(me_vo_event{2, fr, id, {0, 0, 0, 0}});
      obs.erase(it);
      popped_frames.push_back(fr);
      for (auto& x : first)
        if (x == fr) x = fr + 1;
    }
    std::vector<uint8_t> keep(size());
    size_t n2 = 0;
    for (size_t i = 0; i < size(); ++i) {
      keep[i] = !(last[i] < new_first);
      n2 += keep[i];
    }
    if (n2 == size()) return;
    for (size_t i = 0; i < size(); ++i)
      if (!keep[i]) deleted_ids.push_back(ids[i]);
    if (log_events)
      for (int64_t id : deleted_ids) events.push_back(me_vo_event{3, -1, id, {0, 0, 0, 0}});
    remap.assign(size(), -1);
    size_t w = 0;
    for (size_t i = 0; i < size(); ++i) {
      if (!keep[i]) continue;
      remap[i] = (int64_t)w;
      ids[w] = ids[i];
      first[w] = first[i];
      last[w] = last[i];
      active[w] = active[i];
      for (int q = 0; q < 3; ++q) X[3 * w + q] = X[3 * i + q];
      ++w;
    }
    ids.resize(n2);
    first.resize(n2);
    last.resize(n2);
    active.resize(n2);
    X.resize(3 * n2);
    ++gen;
  }

  // The BA window of frames f0..: the rows last seen in it, in table order, with their IDs as the device window's
  // int32 and their landmarks.  False: an ID does not fit int32.
  bool window_rows(int f0, BaRec& rec, std::vector<int32_t>& wid32, std::vector<double>& Xw) const {
    rec.upts.clear();
    rec.wids.clear();
    for (size_t i = 0; i < size(); ++i)
      if (last[i] >= f0) {
        rec.upts.push_back((int64_t)i);
        rec.wids.push_back(ids[i]);
        if (ids[i] >= 2147483647LL) return false;
        wid32.push_back((int32_t)ids[i]);
        Xw.insert(Xw.end(), &X[3 * i], &X[3 * i] + 3);
      }
    rec.gen = gen;
    return true;
  }

  // Where a submitted window's points are now: row j[i], and live[i] = 0 for a track deleted since.  Same
  // generation: the rows as submitted; one compaction on: through remap; further on: by ID.  The loop takes only
  // the first two (one pop at most lies between a window's submit and its result); the third is covered on the
  // host, with an ID still present, deleted, beyond the last row, and an empty table.
  void resolve(const BaRec& ba, std::vector<int64_t>& j, std::vector<uint8_t>& live) const {
    const size_t m = ba.upts.size();
    j.resize(m);
    live.assign(m, 1);
    if (ba.gen == gen) {
      for (size_t i = 0; i < m; ++i) j[i] = ba.upts[i];
    } else if (ba.gen + 1 == gen) {
      for (size_t i = 0; i < m; ++i) {
        const int64_t r = remap[ba.upts[i]];
        live[i] = r >= 0;
        j[i] = std::max<int64_t>(r, 0);
      }
    } else {
      for (size_t i = 0; i < m; ++i) {
        const int64_t r = std::min<int64_t>(find_id(ba.wids[i]), std::max<int64_t>((int64_t)size() - 1, 0));
        live[i] = size() > 0 && ids[r] == ba.wids[i];
        j[i] = r;
      }
    }
  }

  // The residual check's verdict on a solved window (me_vo_loop_set_track_check): the rows given are tracked no
  // further.  They keep their observations and their place in the windows that hold them, and leave by the pops.
  void deactivate(const std::vector<int64_t>& rows) {
    for (int64_t r : rows) active[(size_t)r] = 0;
  }

  // kf_seed: the active tracks' left positions in keyframe t, in table order (the order the next tracker upload
  // has), and with want_xr their x_r there
  void seeded(int t, bool want_xr, std::vector<float>& ref, std::vector<float>& xr) const {
    const FrameObs& po = obs.at(t);
    ref.clear();
    xr.clear();
    for (size_t i = 0; i < size(); ++i) {
      if (!active[i]) continue;
      const size_t pos = (size_t)(std::lower_bound(po.ids.begin(), po.ids.end(), ids[i]) - po.ids.begin());
      ref.push_back(po.feats[4 * pos]);
      ref.push_back(po.feats[4 * pos + 1]);
      if (want_xr) xr.push_back(po.feats[4 * pos + 2]);
    }
  }
};

}  // namespace me_vo
