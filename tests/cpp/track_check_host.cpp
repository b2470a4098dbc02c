// Host program of the residual check's table step (TrackTable::deactivate behind TrackTable::resolve,
// csrc/vo_tracks.hpp alone: no HIP, no libme_hip.so).  A scripted W = 3 run, in the loop's order: flags applied to
// a live row of the same generation, to a row a pop moved between the window's submit and its result, and for a row
// that pop deleted, which are ignored.  tests/test_track_check.py compiles and runs it; it prints one line per case
// and exits 0 when every check held.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../uasl_motion_estimation_amd/csrc/vo_tracks.hpp"

namespace {

using namespace me_vo;

int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// keyframe t: the active rows `cont` (by ID) continue, the others that were active are lost (the loop clears their
// flag in step 4), n_new tracks start
void keyframe(TrackTable& tab, int t, const std::vector<int64_t>& cont, int n_new) {
  std::vector<int64_t> act, trk_idx, fid, new_ids;
  tab.active_rows(act);
  std::vector<float> trk_uv, xr_trk, nuv, nxr;
  for (int64_t r : act) {
    bool goes_on = false;
    for (int64_t id : cont) goes_on |= tab.ids[(size_t)r] == id;
    if (!goes_on) {
      tab.active[(size_t)r] = 0;
      continue;
    }
    trk_idx.push_back(r);
    trk_uv.push_back(100.0f + (float)tab.ids[(size_t)r]);
    trk_uv.push_back(50.0f + (float)t);
    xr_trk.push_back(90.0f + (float)tab.ids[(size_t)r]);
  }
  CHECK(trk_idx.size() == cont.size());  // (every ID asked to continue was active)
  std::vector<uint8_t> nok((size_t)n_new, 1);
  std::vector<double> new_X;
  for (int k = 0; k < n_new; ++k) {
    nuv.push_back(200.0f + (float)k);
    nuv.push_back(60.0f + (float)t);
    nxr.push_back(190.0f + (float)k);
    for (int q = 0; q < 3; ++q) new_X.push_back((double)(tab.latest_id + k) + 0.25 * q);
  }
  tab.book(t, trk_idx, trk_uv, xr_trk, nuv, nxr, nok, new_X, fid, new_ids);
}

// what the loop does with a window's flags (me_vo_loop::ba_finish): the flagged rows still in the table
std::vector<int64_t> apply(TrackTable& tab, const BaRec& rec, const std::vector<uint8_t>& flags,
                           std::vector<int64_t>* applied_ids) {
  std::vector<int64_t> j, rows;
  std::vector<uint8_t> live;
  tab.resolve(rec, j, live);
  for (size_t i = 0; i < rec.upts.size(); ++i)
    if (live[i] && flags[i]) {
      rows.push_back(j[i]);
      applied_ids->push_back(rec.wids[i]);
    }
  tab.deactivate(rows);
  return rows;
}

std::vector<uint8_t> flags_for(const BaRec& rec, const std::vector<int64_t>& ids) {
  std::vector<uint8_t> f(rec.wids.size(), 0);
  for (size_t i = 0; i < rec.wids.size(); ++i)
    for (int64_t id : ids)
      if (rec.wids[i] == id) f[i] = 1;
  return f;
}

std::vector<int64_t> active_ids(const TrackTable& tab) {
  std::vector<int64_t> act, out;
  tab.active_rows(act);
  for (int64_t r : act) out.push_back(tab.ids[(size_t)r]);
  return out;
}

bool frame_has(const TrackTable& tab, int t, int64_t id) {
  const FrameObs& fo = tab.obs.at(t);
  return std::binary_search(fo.ids.begin(), fo.ids.end(), id);
}

}  // namespace

int main() {
  TrackTable tab;
  tab.log_events = true;
  keyframe(tab, 0, {}, 4);         // IDs 0 1 2 3
  keyframe(tab, 1, {1, 2, 3}, 1);  // 0 lost; 4 new
  keyframe(tab, 2, {2, 3, 4}, 1);  // 1 lost; 5 new
  CHECK((active_ids(tab) == std::vector<int64_t>{2, 3, 4, 5}));

  // ---- case 1: window [0, 2] submitted and applied with no pop in between
  BaRec a;
  a.t = 2;
  a.f0 = 0;
  std::vector<int32_t> wid32;
  std::vector<double> Xw;
  CHECK(tab.window_rows(0, a, wid32, Xw));
  CHECK(a.wids.size() == 6 && a.gen == tab.gen);
  const size_t n_events = tab.events.size();
  std::vector<int64_t> applied;
  std::vector<int64_t> rows = apply(tab, a, flags_for(a, {3, 0}), &applied);  // (0 is flagged and inactive already)
  CHECK((applied == std::vector<int64_t>{0, 3}));
  CHECK((rows == std::vector<int64_t>{0, 3}));
  CHECK((active_ids(tab) == std::vector<int64_t>{2, 4, 5}));
  CHECK(tab.events.size() == n_events);         // no event kind of its own
  CHECK(tab.size() == 6 && tab.last[3] == 2 && tab.first[3] == 0);  // the row stays, with what it holds
  CHECK(frame_has(tab, 2, 3));
  std::printf("case1 live_row applied=%zu active=%zu\n", applied.size(), active_ids(tab).size());

  // ---- keyframe 3: the flagged track gets no addMatch, its observations stay
  keyframe(tab, 3, {2, 4, 5}, 1);  // 6 new
  CHECK(!frame_has(tab, 3, 3) && frame_has(tab, 2, 3) && tab.last[3] == 2);
  BaRec b;
  b.t = 3;
  b.f0 = 1;
  wid32.clear();
  Xw.clear();
  CHECK(tab.window_rows(1, b, wid32, Xw));
  CHECK((b.wids == std::vector<int64_t>{1, 2, 3, 4, 5, 6}));  // (3 is still in the window: seen in 1 and 2)

  // ---- cases 2 and 3: a pop between the submit and the result deletes IDs 0 and 1 and moves every other row
  std::vector<int> popped;
  std::vector<int64_t> gone;
  tab.pop(2, popped, gone);
  CHECK((gone == std::vector<int64_t>{0, 1}) && tab.gen == b.gen + 1);
  CHECK((tab.ids == std::vector<int64_t>{2, 3, 4, 5, 6}));
  applied.clear();
  rows = apply(tab, b, flags_for(b, {1, 4}), &applied);
  CHECK((applied == std::vector<int64_t>{4}));      // ID 1 is gone: its flags are ignored
  CHECK((rows == std::vector<int64_t>{2}));         // ID 4 moved from row 4 to row 2
  CHECK((active_ids(tab) == std::vector<int64_t>{2, 5, 6}));  // row 0 (ID 2), where the dead row's index clamps, is untouched
  CHECK(frame_has(tab, 3, 4) && frame_has(tab, 2, 4));
  std::printf("case2 moved_row applied=%zu row=%" PRId64 "\n", applied.size(), rows.empty() ? -1 : rows[0]);
  std::printf("case3 deleted_row ignored=%d\n", (int)(applied.size() == 1));

  // ---- keyframe 4: only the tracks left active go on; the dropped ones leave by the ordinary pops
  keyframe(tab, 4, {2, 5, 6}, 0);
  tab.pop(3, popped, gone);
  CHECK((gone == std::vector<int64_t>{3}));  // last seen in 2
  tab.pop(4, popped, gone);
  CHECK((gone == std::vector<int64_t>{4}));  // last seen in 3
  // an empty list is a no-op
  const std::vector<uint8_t> before = tab.active;
  tab.deactivate({});
  CHECK(tab.active == before);
  std::printf("%s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
