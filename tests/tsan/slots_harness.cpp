// AddressSanitizer / UndefinedBehaviorSanitizer run of kq_slots.hpp and kq::lazy_device (kq_host.hpp) on the CPU, against the
// device-less stand-in for the HIP runtime (mock/hip/hip_runtime.h): a toy slot bank with the shape of kq_wfm / kq_rds /
// kq_fsk's host halves.  A set-up that fails at every one of its runtime objects in turn, the staging of a host-memory
// call, the runs of active slots and the copy-back, and the table's upload.  A second toy bank stands on the frame-grid
// banks' host template (kq_gridbank.hpp, as kq_cw / kq_rtty / kq_psk / kq_ale do): deferred slots (kq::DeferredSlots and
// its flush) and an arena of events (kq::EventArena) -- set, remove and reset with no device, a flush of mixed runs, a flush
// whose set-up fails at every object in turn, the arena's entry points with and without a device.  A third has a history
// and a table of its own, and the shared parts of set and of the getters are checked word for word, symbol_period at both
// edges.  The template's process body launches a kernel and is not part of this run.  LeakSanitizer has the last word:
// whatever a failed set-up or a destroy leaves behind fails the run.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>

#include "kq_gridbank.hpp"

static std::string last_error;
void kq_internal_set_error(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  last_error = buf;
}

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      failures++;                                                      \
    }                                                                  \
  } while (0)

namespace {

constexpr unsigned kMaxSlots = 4096;
constexpr int kObjects = 7;  // what make_device makes: two streams and five allocations

struct ToyPar {
  int active;
  unsigned source;
  int value;
};

struct toy_config {
  int device;
  unsigned max_slots;
  size_t max_samples;
  void *stream;
};

struct toy_bank : kq::HostSide {
  toy_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  struct Dev {
    kq::SlotTable<ToyPar> slots;
    std::map<int, float *> tables;  // as kq_wfm's responses: device memory named from a container
    float *ring = nullptr;
    int *flags = nullptr;
    hipStream_t side = nullptr;
  } d;
};

int make_device(toy_bank *b) {
  auto &d = b->d;
  size_t const S = b->cfg.max_slots;
  if (b->open_stream(b->cfg.stream)) return -1;
  if (d.slots.alloc(*b, S) || b->alloc(&d.ring, S * 16) || b->new_stream(&d.side) || b->alloc(&d.flags, S, true)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

toy_bank *toy_create(unsigned max_slots, size_t max_samples) {
  toy_bank *b = new toy_bank;
  b->cfg = toy_config{0, max_slots, max_samples, nullptr};
  return b;
}

int toy_set(toy_bank *b, unsigned slot, unsigned source, int value) {
  if (!kq::set_args_ok("toy_set", slot, &value, kMaxSlots)) return -1;
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank("toy_set", slot, b->cfg.max_slots)) return -1;
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (kq::lazy_device(b, make_device)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  if (!b->d.tables.count(value)) {
    float *t = nullptr;
    if (b->alloc(&t, 4)) return -1;
    b->d.tables[value] = t;
  }
  b->d.slots.par[slot] = ToyPar{1, source, value};
  return b->d.slots.upload(*b, slot);
}

bool holds_nothing(const toy_bank *b) {
  auto const &d = b->d;
  return !b->dev_ready && b->held.empty() && b->streams.empty() && b->pinned.empty() && b->events.empty() && !b->stream &&
         d.slots.par.empty() && d.slots.all.empty() && !d.slots.d_par && !d.slots.d_list && !d.slots.d_rowmap && !d.slots.d_stage &&
         d.slots.stage_cap == 0 && d.tables.empty() && !d.ring && !d.flags && !d.side;
}

void failed_setup() {
  for (int k = 1; k <= kObjects; k++) {
    toy_bank *b = toy_create(8, 64);
    mock_hip().fail_in = k;
    CHECK(toy_set(b, 2, 0, 7) == -1);
    CHECK(mock_hip().fail_in == 0);  // the k-th object was reached
    CHECK(holds_nothing(b));
    CHECK(kq::remove_slot(b, 2, "toy_remove") == -1 && last_error == "toy_remove: slot 2 holds no decoder");
    CHECK(kq::sync_bank(b, "toy_sync") == 0);
    CHECK(toy_set(b, 2, 0, 7) == 0);  // starts over
    CHECK(b->dev_ready && b->streams.size() == 2 && b->held.size() == 6 && b->d.slots.active(2) && b->d.slots.all == std::vector<int>{2});
    if (k & 1) CHECK(kq::remove_slot(b, 2, "toy_remove") == 0);
    CHECK(kq::destroy_bank(b, "toy_destroy") == 0);
  }
  // one that never got its device, destroyed as it is
  toy_bank *b = toy_create(8, 64);
  mock_hip().fail_in = 3;
  CHECK(toy_set(b, 0, 0, 1) == -1 && holds_nothing(b));
  CHECK(kq::destroy_bank(b, "toy_destroy") == 0);
  mock_hip().fail_in = kObjects + 1;  // past the set-up: toy_set's own allocation fails, the device half stays
  b = toy_create(8, 64);
  CHECK(toy_set(b, 0, 0, 1) == -1 && mock_hip().fail_in == 0);
  CHECK(b->dev_ready && b->held.size() == 5 && b->d.slots.all.empty());
  CHECK(toy_set(b, 0, 0, 1) == 0);
  CHECK(kq::destroy_bank(b, "toy_destroy") == 0);
}

template <class T>
void staging_of(toy_bank *b, bool first) {
  unsigned const block_len = 5, nblocks = 3;
  size_t const row_stride = 7, src_stride = 24, rows = 6, ncall = block_len * nblocks;
  std::vector<T> src(rows * src_stride);
  for (size_t i = 0; i < src.size(); i++) src[i] = (T)(1000 + i);
  auto &t = b->d.slots;
  int const mallocs = mock_hip().mallocs, copies2d = mock_hip().copies2d;
  kq::Staged in{};
  CHECK(t.stage_rows(*b, src.data(), sizeof(T), src_stride, row_stride, block_len, nblocks, b->cfg.max_samples * 4, &in) == 0);
  CHECK(mock_hip().mallocs == mallocs + (first ? 1 : 0));  // grow: once, and not again at the same size
  CHECK(mock_hip().copies2d == copies2d + 3);              // one copy per distinct row
  CHECK((t.rowmap == std::vector<int>{0, 1, 0, 2}));
  CHECK(t.stage_cap == 3 * b->cfg.max_samples * 4);
  CHECK(in.src == t.d_stage && in.src_stride == ncall && in.row_stride == block_len && in.rowmap == t.d_rowmap);
  for (size_t i = 0; i < 4; i++) CHECK(t.d_rowmap[i] == t.rowmap[i]);
  unsigned const source_of_row[3] = {5, 2, 0};
  const T *stage = reinterpret_cast<const T *>(t.d_stage);
  for (size_t r = 0; r < 3; r++)
    for (size_t k = 0; k < nblocks; k++)
      for (size_t j = 0; j < block_len; j++)
        CHECK(stage[r * ncall + k * block_len + j] == src[source_of_row[r] * src_stride + k * row_stride + j]);
  // one block: the row stride does not count
  CHECK(t.stage_rows(*b, src.data(), sizeof(T), src_stride, 0, block_len, 1, b->cfg.max_samples * 4, &in) == 0);
  for (size_t j = 0; j < block_len; j++) CHECK(stage[2 * block_len + j] == src[0 * src_stride + j]);
}

std::vector<std::pair<size_t, size_t>> runs_of(const toy_bank *b) {
  std::vector<std::pair<size_t, size_t>> r;
  CHECK(b->d.slots.for_runs([&](size_t s0, size_t n) {
    r.emplace_back(s0, n);
    return 0;
  }) == 0);
  return r;
}

void table_staging_runs() {
  using Runs = std::vector<std::pair<size_t, size_t>>;
  unsigned const S = 8;
  toy_bank *b = toy_create(S, 15);
  auto &t = b->d.slots;
  CHECK(runs_of(b).empty());
  // set, remove, set on mixed slots: {0, 1, 3, 6} on sources {5, 2, 5, 0}
  CHECK(toy_set(b, 6, 9, 60) == 0 && toy_set(b, 1, 2, 10) == 0 && toy_set(b, 4, 1, 40) == 0 && toy_set(b, 3, 5, 30) == 0);
  CHECK(kq::remove_slot(b, 4, "toy_remove") == 0 && kq::remove_slot(b, 6, "toy_remove") == 0);
  CHECK(toy_set(b, 0, 5, 0) == 0 && toy_set(b, 6, 0, 61) == 0);
  CHECK((t.all == std::vector<int>{0, 1, 3, 6}));
  for (size_t i = 0; i < t.all.size(); i++) CHECK(t.d_list[i] == t.all[i]);
  for (unsigned s = 0; s < S; s++) {
    CHECK(t.d_par[s].active == t.par[s].active && t.d_par[s].source == t.par[s].source && t.d_par[s].value == t.par[s].value);
    CHECK(t.active(s) == (s == 0 || s == 1 || s == 3 || s == 6));
  }
  CHECK(t.par[6].value == 61 && t.par[6].source == 0 && t.par[4].value == 0 && !t.active(S) && !t.active(kMaxSlots));
  // the entry points' checks, word for word
  CHECK(toy_set(b, S, 0, 0) == -1 && last_error == "toy_set: slot 8 >= max_slots 8");
  CHECK(toy_set(b, kMaxSlots, 0, 0) == -1 && last_error == "toy_set: slot 4096 is beyond any bank (4096 slots at most)");
  CHECK(!kq::set_args_ok("toy_set", 0, nullptr, kMaxSlots) && last_error == "toy_set: null params");
  CHECK(kq::remove_slot(b, 4, "toy_remove") == -1 && last_error == "toy_remove: slot 4 holds no decoder");
  CHECK(kq::remove_slot((toy_bank *)nullptr, 4, "toy_remove") == -1 && last_error == "toy_remove: null bank");
  CHECK(kq::sync_bank((toy_bank *)nullptr, "toy_sync") == -1 && last_error == "toy_sync: null bank");
  CHECK(kq::destroy_bank((toy_bank *)nullptr, "toy_destroy") == -1 && last_error == "toy_destroy: null bank");
  CHECK(!kq::blocks_ok("toy_process", 15, 7, 4, 4) && last_error == "toy_process: nblocks 4 x block_len 4 = 16 > max_samples 15");
  CHECK(!kq::blocks_ok("toy_process", 15, 4, 5, 3) && last_error == "toy_process: row_stride 4 < block_len 5");
  CHECK(kq::blocks_ok("toy_process", 15, 0, 15, 1) && kq::blocks_ok("toy_process", 15, 5, 5, 3));
  CHECK(kq::call_work(b, "toy_process", 0, nullptr, "src") == kq::CALL_EMPTY);
  CHECK(kq::call_work(b, "toy_process", 15, nullptr, "src") == kq::CALL_FAILED && last_error == "toy_process: null src");
  CHECK(kq::call_work(b, "toy_process", 15, b, "src") == kq::CALL_RUN);

  staging_of<float>(b, true);
  staging_of<int16_t>(b, false);

  CHECK((runs_of(b) == Runs{{0, 2}, {3, 1}, {6, 1}}));
  // copy-back: rows of 4 on the device, rows of 6 on the host, 3 elements of each active row
  {
    std::vector<uint16_t> dev(S * 4), host(S * 6, 0xFFFF);
    for (size_t i = 0; i < dev.size(); i++) dev[i] = (uint16_t)i;
    uint16_t *d_plane = nullptr;
    CHECK(b->alloc(&d_plane, dev.size()) == 0);
    memcpy(d_plane, dev.data(), dev.size() * sizeof(uint16_t));
    CHECK(t.for_runs([&](size_t s0, size_t n) { return kq::copy_rows_back(*b, host.data(), 6, d_plane, 4, 3, sizeof(uint16_t), s0, n); }) == 0);
    for (size_t s = 0; s < S; s++)
      for (size_t j = 0; j < 6; j++) CHECK(host[s * 6 + j] == (t.active((unsigned)s) && j < 3 ? dev[s * 4 + j] : 0xFFFF));
    // a run that fails ends the walk
    int calls = 0;
    CHECK(t.for_runs([&](size_t, size_t) { return ++calls == 2 ? -1 : 0; }) == -1 && calls == 2);
  }
  for (unsigned s : {2u, 4u, 5u, 7u}) CHECK(toy_set(b, s, s, 0) == 0);
  CHECK((runs_of(b) == Runs{{0, 8}}));
  // the last slot to go: its entry is copied, the (empty) list is not
  for (unsigned s = 0; s < S - 1; s++) CHECK(kq::remove_slot(b, s, "toy_remove") == 0);
  CHECK((t.all == std::vector<int>{7}) && t.d_list[0] == 7);
  int const copies = mock_hip().copies;
  CHECK(kq::remove_slot(b, 7, "toy_remove") == 0);
  CHECK(mock_hip().copies == copies + 1 && t.all.empty() && t.d_par[7].active == 0 && t.d_list[0] == 7);
  CHECK(runs_of(b).empty());
  CHECK(kq::call_work(b, "toy_process", 15, b, "src") == kq::CALL_IDLE);
  CHECK(kq::destroy_bank(b, "toy_destroy") == 0);
}

// ---- a second toy bank, on the frame-grid banks' host template (kq_gridbank.hpp: kq_cw / kq_rtty / kq_psk / kq_ale's host
// halves): deferred slots and an arena of events, a cold start that is not all zero, no history ------------------------------
namespace tc = kq::tonecorr;
constexpr int kDefObjects = 8;  // what GridBank::make_device makes here: a stream and seven allocations

struct DefPar {
  int active;
  unsigned source;  // (def_set: the slot's own number)
  int value;
};

struct DefEvent {
  unsigned code, slot;
};

struct DefGeom {
  tc::FrameGrid grid;
  unsigned warm, snr;
  unsigned long long min_p;
  int max_events;
};

struct def_config {
  int device;
  unsigned max_slots;
  size_t max_samples;
  void *stream;
  unsigned block_len, warm, snr, max_events;
  unsigned long long min_p;
};

// The slots that were started cold, consecutive ones merged.  The template's cold hook sees one slot at a time, so this
// says which slots flush() started cold, not where it split its runs (two runs of set slots never touch, so the two agree
// wherever flush() is right); the counts of copies below are what still sees the runs.
std::vector<std::pair<size_t, size_t>> colds;

struct DefKind {
  using Config = def_config;
  using Geom = DefGeom;
  using Par = DefPar;
  using Status = int;  // [S]: the slot's value at its cold start
  using Event = DefEvent;
  using Hist = void;
  using Tables = tc::NoTables;
  static constexpr bool kZeroCold = false;
  static void cold(DefPar const &p, int &r) {  // as kq_cw's records: host memory that a run is copied from
    if (!colds.empty() && colds.back().first + colds.back().second == p.source) colds.back().second++;
    else colds.emplace_back(p.source, 1);
    r = p.value;
  }
};

struct def_bank : tc::GridBank<DefKind> {};

def_bank *def_create(unsigned max_slots) {
  def_config const cfg{0, max_slots, 64, nullptr, 24, 3, 16, 4, 5};
  def_bank *b = tc::finish_create<def_bank>(&cfg, 3200);
  CHECK(b->g.grid.B == 24 && b->g.grid.Bs == 26 && b->Lmin == 1 && b->g.warm == 3 && b->g.snr == 16 && b->g.min_p == 5 &&
        b->g.max_events == 4 && b->cfg.max_slots == max_slots && b->def.want.size() == max_slots);
  return b;
}

void def_set(def_bank *b, unsigned slot, int value) {
  std::unique_lock<std::mutex> lk;
  CHECK(tc::open_set(b, "toy_set", slot, &value, kMaxSlots, lk) && lk.owns_lock());
  b->def.set(slot, DefPar{1, slot, value});
}

bool def_holds_nothing(const def_bank *b) {
  auto const &d = b->d;
  return !b->dev_ready && b->held.empty() && b->streams.empty() && !b->stream && d.slots.par.empty() && d.slots.all.empty() &&
         !d.slots.d_par && !d.slots.d_list && !d.slots.d_rowmap && !d.table && !d.state && !d.hist && !d.arena.ev && !d.arena.n &&
         d.arena.cap == 0 && !d.st;
}

// what a kernel would have filed: n events in the slot's arena
void def_file(def_bank *b, unsigned slot, unsigned n) {
  for (unsigned i = 0; i < n; i++) b->d.arena.ev[slot * b->d.arena.cap + i] = DefEvent{100 * slot + i, slot};
  b->d.arena.n[slot] = n;
}

void deferred_without_a_device() {
  unsigned const S = 8;
  colds.clear();
  def_bank *b = def_create(S);
  int const mallocs = mock_hip().mallocs, copies = mock_hip().copies;
  std::optional<kq::DeviceScope> scope;
  // set, remove and reset touch no device; with no slot left that wants one, neither do the entry points that read it
  def_set(b, 1, 10);
  def_set(b, 2, 20);
  def_set(b, 2, 21);
  CHECK(b->def.nwant == 2 && (b->def.dirty == std::vector<unsigned>{1, 2}) && b->def.is_set(2) && !b->def.is_set(3) && !b->def.is_set(S));
  CHECK(kq::deferred_remove(b, 3, "toy_remove") == -1 && last_error == "toy_remove: slot 3 holds no decoder");
  CHECK(kq::deferred_remove(b, S, "toy_remove") == -1 && last_error == "toy_remove: slot 8 holds no decoder");
  CHECK(kq::deferred_remove((def_bank *)nullptr, 1, "toy_remove") == -1 && last_error == "toy_remove: null bank");
  CHECK(kq::deferred_remove(b, 1, "toy_remove") == 0 && kq::deferred_remove(b, 2, "toy_remove") == 0 && b->def.nwant == 0);
  b->n_cur = 99;
  CHECK(kq::deferred_reset(b, "toy_reset") == 0 && b->n_cur == 0 && b->def.dirty.size() == 2);
  CHECK(kq::deferred_reset((def_bank *)nullptr, "toy_reset") == -1 && last_error == "toy_reset: null bank");
  std::vector<uint32_t> counts(S, 0xFFFFFFFFu);
  CHECK(kq::pull_counts(b, "toy_pull_counts", counts.data()) == 0 && counts == std::vector<uint32_t>(S, 0u));
  CHECK(b->def.dirty.empty() && !b->def.is_dirty[1] && !b->def.is_dirty[2]);  // forgotten: there was nowhere to bring them
  DefEvent e{7, 7};
  CHECK(kq::pull_event(b, "toy_pull_event", 1, 0, &e) == -1 && last_error == "toy_pull_event: slot 1 has 0 events" && e.code == 7);
  CHECK(kq::pull_event(b, "toy_pull_event", S, 0, &e) == -1 && last_error == "toy_pull_event: slot 8 >= max_slots 8");
  CHECK(kq::pull_event(b, "toy_pull_event", 1, 0, (DefEvent *)nullptr) == -1 && last_error == "toy_pull_event: null event");
  CHECK(kq::pull_counts(b, "toy_pull_counts", nullptr) == -1 && last_error == "toy_pull_counts: null counts");
  CHECK(kq::pull_counts((def_bank *)nullptr, "toy_pull_counts", counts.data()) == -1 && last_error == "toy_pull_counts: null bank");
  CHECK(kq::clear_arena(b, "toy_clear") == 0);
  CHECK(kq::clear_arena((def_bank *)nullptr, "toy_clear") == -1 && last_error == "toy_clear: null bank");
  CHECK(kq::begin_call(b, "toy_process", 0, b, scope) == kq::CALL_EMPTY && b->n_cur == 0);
  CHECK(kq::begin_call(b, "toy_process", 15, nullptr, scope) == kq::CALL_FAILED && last_error == "toy_process: null src");
  CHECK(kq::begin_call(b, "toy_process", 15, b, scope) == kq::CALL_IDLE && b->n_cur == 15 && !scope);
  CHECK(def_holds_nothing(b) && mock_hip().mallocs == mallocs && mock_hip().copies == copies && colds.empty());
  CHECK(kq::destroy_bank(b, "toy_destroy") == 0);
}

void deferred_flush_and_arena() {
  using Runs = std::vector<std::pair<size_t, size_t>>;
  unsigned const S = 8;
  colds.clear();
  def_bank *b = def_create(S);
  auto &t = b->d.slots;
  // before the first call: 0, 1, 2 together, 4 alone, 3 set and removed again in the middle
  def_set(b, 4, 40);
  def_set(b, 0, 5);
  def_set(b, 3, 30);
  def_set(b, 1, 10);
  def_set(b, 2, 20);
  CHECK(kq::deferred_remove(b, 3, "toy_remove") == 0 && b->def.nwant == 4 && def_holds_nothing(b));
  std::vector<uint32_t> counts(S, 0xFFFFFFFFu);
  int copies = mock_hip().copies;
  CHECK(kq::pull_counts(b, "toy_pull_counts", counts.data()) == 0 && counts == std::vector<uint32_t>(S, 0u));
  CHECK(b->dev_ready && b->held.size() == 7 && b->streams.size() == 1 && b->def.dirty.empty());
  CHECK((colds == Runs{{0, 3}, {4, 1}}));
  // the cosine table (the template's set-up sends it), three runs of parameters, two cold starts, upload's record and list,
  // the counts
  CHECK(mock_hip().copies == copies + 1 + 3 + 2 + 2 + 1);
  CHECK(std::memcmp(b->d.table, tc::cos_table().data(), tc::kTable * sizeof(short)) == 0);
  CHECK((t.all == std::vector<int>{0, 1, 2, 4}));
  for (size_t i = 0; i < t.all.size(); i++) CHECK(t.d_list[i] == t.all[i]);
  for (unsigned s = 0; s < S; s++) {
    bool const set = s < 3 || s == 4;
    CHECK(t.d_par[s].active == (set ? 1 : 0) && t.d_par[s].value == b->def.want[s].value && t.d_par[s].source == (set ? s : 0));
    CHECK(b->d.state[s] == b->def.want[s].value);
  }
  CHECK(b->d.state[0] == 5 && b->d.state[4] == 40 && b->d.state[3] == 0);
  // events, and the index past them
  def_file(b, 0, 2);
  def_file(b, 2, 4);
  DefEvent e{7, 7};
  CHECK(kq::pull_event(b, "toy_pull_event", 0, 2, &e) == -1 && last_error == "toy_pull_event: slot 0 has 2 events" && e.code == 7);
  CHECK(kq::pull_event(b, "toy_pull_event", 0, 1, &e) == 0 && e.code == 1 && e.slot == 0);
  CHECK(kq::pull_event(b, "toy_pull_event", 2, 3, &e) == 0 && e.code == 203 && e.slot == 2);
  CHECK(kq::pull_event(b, "toy_pull_event", 3, 0, &e) == -1 && last_error == "toy_pull_event: slot 3 has 0 events");
  // a slot set again starts cold with an empty arena, a removed one keeps its arena; the others are left alone
  def_set(b, 2, 22);
  CHECK(kq::deferred_remove(b, 0, "toy_remove") == 0);
  colds.clear();
  CHECK(kq::pull_counts(b, "toy_pull_counts", counts.data()) == 0 && (counts == std::vector<uint32_t>{2, 0, 0, 0, 0, 0, 0, 0}));
  CHECK((colds == Runs{{2, 1}}) && b->d.state[2] == 22 && b->d.state[1] == 10 && (t.all == std::vector<int>{1, 2, 4}));
  CHECK(t.d_par[0].active == 0 && t.d_par[2].value == 22);
  // reset: every slot that is set starts cold again, in runs
  def_file(b, 1, 1);
  colds.clear();
  b->n_cur = 5;
  CHECK(kq::deferred_reset(b, "toy_reset") == 0 && b->n_cur == 0);
  std::optional<kq::DeviceScope> scope;
  CHECK(kq::begin_call(b, "toy_process", 15, b, scope) == kq::CALL_RUN && b->n_cur == 0 && scope);
  CHECK((colds == Runs{{1, 2}, {4, 1}}) && b->d.arena.n[1] == 0 && b->d.arena.n[0] == 2);
  // the status records of a host-memory call: the bank's own plane at stride 1, the active slots' rows back
  {
    std::vector<int> host(S * 2, -1);
    int *st = nullptr;
    size_t stride = 0;
    CHECK(kq::bind_status(b, 1, host.data(), (size_t)2, &st, &stride) == 0 && st == host.data() && stride == 2);
    CHECK(kq::bind_status(b, 0, (int *)nullptr, (size_t)2, &st, &stride) == 0 && st == nullptr && stride == 1);
    CHECK(kq::bind_status(b, 0, host.data(), (size_t)2, &st, &stride) == 0 && st == b->d.st && stride == 1);
    for (unsigned s = 0; s < S; s++) b->d.st[s] = 1000 + (int)s;
    CHECK(kq::end_host_call(b, host.data(), (size_t)2, nullptr) == 0);
    for (unsigned s = 0; s < S; s++) CHECK(host[2 * s] == (t.active(s) ? 1000 + (int)s : -1) && host[2 * s + 1] == -1);
    int more = 0;
    CHECK(kq::end_host_call(b, (int *)nullptr, (size_t)2, [&](size_t, size_t n) { return more += (int)n, 0; }) == 0 && more == 3);
  }
  // clear: every arena empty, the slots as they were
  CHECK(kq::clear_arena(b, "toy_clear") == 0);
  CHECK(kq::pull_counts(b, "toy_pull_counts", counts.data()) == 0 && counts == std::vector<uint32_t>(S, 0u));
  CHECK((t.all == std::vector<int>{1, 2, 4}));
  CHECK(kq::destroy_bank(b, "toy_destroy") == 0);
}

void deferred_failed_setup() {
  unsigned const S = 8;
  for (int k = 1; k <= kDefObjects; k++) {
    colds.clear();
    def_bank *b = def_create(S);
    def_set(b, 2, 7);
    def_set(b, 3, 8);
    std::vector<uint32_t> counts(S, 0xFFFFFFFFu);
    mock_hip().fail_in = k;
    CHECK(kq::pull_counts(b, "toy_pull_counts", counts.data()) == -1);
    CHECK(mock_hip().fail_in == 0);  // the k-th object was reached
    CHECK(def_holds_nothing(b) && b->def.dirty.size() == 2 && b->def.nwant == 2 && colds.empty());
    CHECK(counts[0] == 0xFFFFFFFFu);
    DefEvent e{7, 7};
    if (k & 1) {  // the next entry point starts over
      CHECK(kq::pull_event(b, "toy_pull_event", 2, 0, &e) == -1 && last_error == "toy_pull_event: slot 2 has 0 events");
    } else {
      CHECK(kq::pull_counts(b, "toy_pull_counts", counts.data()) == 0 && counts == std::vector<uint32_t>(S, 0u));
    }
    CHECK(b->dev_ready && b->held.size() == 7 && b->def.dirty.empty() && (b->d.slots.all == std::vector<int>{2, 3}));
    CHECK(b->d.state[2] == 7 && b->d.state[3] == 8 && colds.size() == 1);
    CHECK(kq::destroy_bank(b, "toy_destroy") == 0);
  }
  // one whose device never came, destroyed with its slots still waiting
  def_bank *b = def_create(S);
  def_set(b, 0, 1);
  std::optional<kq::DeviceScope> scope;
  mock_hip().fail_in = 4;
  CHECK(kq::begin_call(b, "toy_process", 15, b, scope) == kq::CALL_FAILED && def_holds_nothing(b) && b->n_cur == 0);
  CHECK(kq::destroy_bank(b, "toy_destroy") == 0);
}

// ---- a third, as kq_ale's: a history window, a table of its own, and a cold start that is all zero --------------------------
constexpr int kWinObjects = 10;  // a stream and nine allocations

struct WinTables {
  short *extra = nullptr;
  int make(kq::HostSide &h) {
    if (h.alloc(&extra, 16)) return -1;
    short const ones[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    KQ_TRY(hipMemcpyAsync(extra, ones, sizeof ones, hipMemcpyHostToDevice, h.stream));  // (the mock copies at once)
    return 0;
  }
};

struct WinKind : DefKind {
  using Hist = tc::FrameHist<2>;
  using Tables = WinTables;
  static constexpr bool kZeroCold = true;
};

struct win_bank : tc::GridBank<WinKind> {};

void windowed_bank() {
  unsigned const S = 8;
  def_config const cfg{0, S, 64, nullptr, 48, 0, 16, 4, 0};
  std::vector<uint32_t> counts(S);
  for (int k = 0; k <= kWinObjects; k++) {  // 0: nothing fails
    win_bank *b = tc::finish_create<win_bank>(&cfg, 3200);
    CHECK(b->g.grid.Bs == 50 && b->Lmin == 1);
    std::unique_lock<std::mutex> lk;
    int v = 0;
    CHECK(tc::open_set(b, "toy_set", 1, &v, kMaxSlots, lk));
    b->def.set(1, DefPar{1, 1, 11});
    b->def.set(2, DefPar{1, 2, 12});
    lk.unlock();
    mock_hip().fail_in = k;
    if (k) {
      CHECK(kq::pull_counts(b, "toy_pull_counts", counts.data()) == -1 && mock_hip().fail_in == 0);
      CHECK(!b->dev_ready && b->held.empty() && b->streams.empty() && !b->d.table && !b->d.tables.extra && !b->d.state && !b->d.hist);
    }
    CHECK(kq::pull_counts(b, "toy_pull_counts", counts.data()) == 0 && b->dev_ready && b->held.size() == 9);
    CHECK(b->d.tables.extra[15] == 1 && b->d.table[0] == 32767);
    // what a call would leave; a slot set again starts from zeros, record and history, its neighbour keeps both
    for (unsigned s = 1; s <= 2; s++) {
      b->d.state[s] = 100 + (int)s;
      for (int t = 0; t < 2; t++)
        for (int i = 0; i < tc::kHist; i++) b->d.hist[s].v[t][i] = 7;
    }
    CHECK(tc::open_set(b, "toy_set", 2, &v, kMaxSlots, lk));
    b->def.set(2, DefPar{1, 2, 13});
    lk.unlock();
    CHECK(kq::pull_counts(b, "toy_pull_counts", counts.data()) == 0);
    CHECK(b->d.state[1] == 101 && b->d.state[2] == 0 && b->d.hist[1].v[1][tc::kHist - 1] == 7);
    for (int t = 0; t < 2; t++)
      for (int i = 0; i < tc::kHist; i++) CHECK(b->d.hist[2].v[t][i] == 0);
    CHECK(kq::destroy_bank(b, "toy_destroy") == 0);
  }
}

// the shared parts of kq_*_set and the getters' opening, word for word
void set_and_get_openings() {
  def_bank *b = def_create(8);
  int v = 0;
  {
    std::unique_lock<std::mutex> lk;
    CHECK(!tc::open_set(b, "toy_set", kMaxSlots, &v, kMaxSlots, lk) && last_error == "toy_set: slot 4096 is beyond any bank (4096 slots at most)");
    CHECK(!tc::open_set(b, "toy_set", 0, nullptr, kMaxSlots, lk) && last_error == "toy_set: null params" && !lk.owns_lock());
    CHECK(!tc::open_set((def_bank *)nullptr, "toy_set", 0, &v, kMaxSlots, lk) && last_error == "toy_set: null bank" && !lk.owns_lock());
    CHECK(!tc::open_set(b, "toy_set", 8, &v, kMaxSlots, lk) && last_error == "toy_set: slot 8 >= max_slots 8" && lk.owns_lock());
  }
  CHECK(tc::tone_ok("toy_set", 12000.0, 1000.0, "pitch %g", 1000.0) && tc::tone_ok("toy_set", 12000.0, 5999.9, "mark %g", 5999.9));
  CHECK(!tc::tone_ok("toy_set", 12000.0, 0.0, "mark %g", 0.0) && last_error == "toy_set: mark 0 must be above 0 and below samprate / 2");
  CHECK(!tc::tone_ok("toy_set", 12000.0, 6000.0, "space %g", 6000.0) && last_error == "toy_set: space 6000 must be above 0 and below samprate / 2");
  CHECK(!tc::tone_ok("toy_set", 12000.0, std::nan(""), "pitch %g", 1.5) && last_error == "toy_set: pitch 1.5 must be above 0 and below samprate / 2");
  CHECK(!tc::tone_ok("toy_set", 12000.0, -250.0, "tone %d at %g (f0 %g, df %g)", 7, -250.0, 1500.0, -250.0) &&
        last_error == "toy_set: tone 7 at -250 (f0 1500, df -250) must be above 0 and below samprate / 2");
  // tb = rint(256 Fs / (B baud)) = rint(128000 / baud) at both edges of 2048..8192
  int tb = -1, W = -1;
  CHECK(tc::symbol_period("toy_set", 12000.0, 24, 128000.0 / 2048.0, "bit", &tb, &W) && tb == 2048 && W == 8);
  CHECK(tc::symbol_period("toy_set", 12000.0, 24, 128000.0 / 8192.0, "symbol", &tb, &W) && tb == 8192 && W == 32);
  CHECK(tc::symbol_period("toy_set", 12000.0, 24, 128000.0 / 2047.6, "bit", &tb, &W) && tb == 2048 && W == 8);
  CHECK(tc::symbol_period("toy_set", 12000.0, 24, 128000.0 / 8192.4, "bit", &tb, &W) && tb == 8192 && W == 32);
  CHECK(tc::symbol_period("toy_set", 12000.0, 24, 45.45, "bit", &tb, &W) && tb == 2816 && W == 11);
  tb = W = -1;
  CHECK(!tc::symbol_period("toy_set", 12000.0, 24, 128000.0 / 2047.4, "bit", &tb, &W) && tb == -1 && W == -1);
  CHECK(last_error.find("toy_set: baud 62.5") == 0 &&
        last_error.find(" makes tb 2047, a bit of 7.99609 frames of 24 samples, outside 2048..8192 (8 to 32 frames)") != std::string::npos);
  CHECK(!tc::symbol_period("toy_set", 12000.0, 24, 128000.0 / 8192.6, "symbol", &tb, &W) && tb == -1 && W == -1);
  CHECK(last_error.find(" makes tb 8193, a symbol of 32.0039 frames of 24 samples, outside 2048..8192 (8 to 32 frames)") != std::string::npos);
  CHECK(!tc::symbol_period("toy_set", 12000.0, 24, 0.0, "bit", &tb, &W) && last_error == "toy_set: baud 0 must be positive and finite");
  CHECK(!tc::symbol_period("toy_set", 12000.0, 24, INFINITY, "bit", &tb, &W) && last_error == "toy_set: baud inf must be positive and finite");
  CHECK(!tc::symbol_period("toy_set", 12000.0, 24, std::nan(""), "bit", &tb, &W) && tb == -1);
  // the getters
  def_set(b, 3, 33);
  {
    std::unique_lock<std::mutex> lk;
    CHECK(!tc::wanted((def_bank *)nullptr, "toy_get", 3, &v, "out", lk) && last_error == "toy_get: null bank");
    CHECK(!tc::wanted(b, "toy_get", 3, nullptr, "inc", lk) && last_error == "toy_get: null inc" && !lk.owns_lock());
    CHECK(!tc::wanted(b, "toy_get", 4, &v, "out", lk) && last_error == "toy_get: slot 4 holds no decoder");
  }
  {
    std::unique_lock<std::mutex> lk;
    CHECK(!tc::wanted(b, "toy_get", 8, &v, "out", lk) && last_error == "toy_get: slot 8 holds no decoder");
  }
  {
    std::unique_lock<std::mutex> lk;
    const DefPar *w = tc::wanted(b, "toy_get", 3, &v, "out", lk);
    CHECK(w && w->value == 33 && w->source == 3 && lk.owns_lock());
  }
  CHECK(def_holds_nothing(b));  // none of it touched a device
  CHECK(kq::destroy_bank(b, "toy_destroy") == 0);
}

}  // namespace

int main() {
  failed_setup();
  table_staging_runs();
  deferred_without_a_device();
  deferred_flush_and_arena();
  deferred_failed_setup();
  windowed_bank();
  set_and_get_openings();
  if (failures) {
    fprintf(stderr, "slot banks' host layer: %d checks failed\n", failures);
    return 1;
  }
  printf("slot banks' host layer: ok\n");
  return 0;
}
