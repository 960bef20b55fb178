// CPU test of the device solver's call-order state (lpopc_amd/csrc/rpm_ipm_hold.hpp) against the four flags it replaced: every
// sequence of calls up to DEPTH, each call with each of its outcomes, on IpmHold and on a literal restatement of the flags and
// their assignments; after every call every predicate equals the flag expression it replaced.  Compiled and run by
// tests/test_ipm_hold_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "../../lpopc_amd/csrc/rpm_ipm_hold.hpp"

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
  } while (0)

using rpm::IpmHold;

// The flags as rpm_ipm held them and as its entry points assigned them.  One difference, on purpose: rpm_ipm_debug_start used to
// leave debug_started and debug_ls alone until it had succeeded, so a start that failed on the device kept them; here it clears
// them when it begins.
struct Flags {
  bool solved = false, debug_started = false, state_held = false;
  int debug_ls = 0;
};

enum Call {
  SOLVE_OK, SOLVE_FAILS, FACTOR_HOOK, LBFGS_STEP_HOOK, START_OK, START_FAILS, PASS_DIRECTION, PASS_NO_DIRECTION, PASS_FAILS,
  LINE_SEARCH_OK, LINE_SEARCH_FAILS, UPDATE, SENSITIVITIES, SENSITIVITY_RHS, BOUND_MULTIPLIERS, N_CALLS
};

// -> the call was accepted (a refused call changes nothing)
static bool call_flags(Flags& f, Call c, bool* first_round) {
  switch (c) {
    case SOLVE_OK: case SOLVE_FAILS:
      f.debug_started = false; f.state_held = false; f.debug_ls = 0;        // ipm_solve_dev, entry
      if (c == SOLVE_OK) { f.solved = true; f.state_held = true; }          // IpmLoop::collect
      return true;
    case FACTOR_HOOK: case LBFGS_STEP_HOOK:
      f.debug_started = false; f.state_held = false; f.debug_ls = 0;
      return true;
    case START_OK: case START_FAILS:
      f.solved = false; f.state_held = false;
      f.debug_started = false; f.debug_ls = 0;                              // (the one difference)
      if (c == START_OK) { f.debug_started = true; f.state_held = true; f.debug_ls = 0; }
      return true;
    case PASS_DIRECTION: case PASS_NO_DIRECTION: case PASS_FAILS:
      if (!f.debug_started) return false;
      f.debug_started = false; f.debug_ls = 0;
      if (c != PASS_FAILS) f.debug_ls = c == PASS_DIRECTION ? 1 : 0;
      return true;
    case LINE_SEARCH_OK: case LINE_SEARCH_FAILS:
      if (f.debug_ls == 0) return false;
      *first_round = f.debug_ls == 1;
      f.debug_ls = 0; f.state_held = false;
      if (c == LINE_SEARCH_OK) f.debug_ls = 2;
      return true;
    case UPDATE:
      if (f.debug_ls != 2) return false;
      f.debug_ls = 0;
      return true;
    case SENSITIVITIES:
      if (!f.state_held) return false;
      f.debug_ls = 0;
      return true;
    case SENSITIVITY_RHS: return f.state_held;
    case BOUND_MULTIPLIERS: return f.solved;
    default: return false;
  }
}

static bool call_hold(IpmHold& h, Call c, bool* first_round) {
  switch (c) {
    case SOLVE_OK: case SOLVE_FAILS:
      h.solve_begins();
      if (c == SOLVE_OK) h.solve_ends();
      return true;
    case FACTOR_HOOK: case LBFGS_STEP_HOOK: h.overwritten(); return true;
    case START_OK: case START_FAILS:
      h.start_begins();
      if (c == START_OK) h.start_ends();
      return true;
    case PASS_DIRECTION: case PASS_NO_DIRECTION: case PASS_FAILS:
      if (!h.pass_allowed()) return false;
      h.pass_begins();
      if (c != PASS_FAILS) h.pass_ends(c == PASS_DIRECTION);
      return true;
    case LINE_SEARCH_OK: case LINE_SEARCH_FAILS:
      if (!h.line_search_allowed()) return false;
      *first_round = h.line_search_begins();
      if (c == LINE_SEARCH_OK) h.line_search_ends();
      return true;
    case UPDATE:
      if (!h.update_allowed()) return false;
      h.updated();
      return true;
    case SENSITIVITIES:
      if (!h.holds_state()) return false;
      h.sensitivities_taken();
      return true;
    case SENSITIVITY_RHS: return h.holds_state();
    case BOUND_MULTIPLIERS: return h.multipliers_ready();
    default: return false;
  }
}

// the table of DESIGN.md f-2: the flags every state stands for
static void check_same(const IpmHold& h, const Flags& f) {
  CHECK(h.pass_allowed() == f.debug_started);
  CHECK(h.line_search_allowed() == (f.debug_ls != 0));
  CHECK(h.update_allowed() == (f.debug_ls == 2));
  CHECK(h.holds_state() == f.state_held);
  CHECK(h.multipliers_ready() == f.solved);
  const int ds = f.debug_started, sh = f.state_held, ls = f.debug_ls;
  switch (h.state) {
    case IpmHold::Nothing: CHECK(ds == 0 && sh == 0 && ls == 0); break;
    case IpmHold::Started: CHECK(ds == 1 && sh == 1 && ls == 0); break;
    case IpmHold::Held: CHECK(ds == 0 && sh == 1 && ls == 0); break;
    case IpmHold::Direction: CHECK(ds == 0 && sh == 1 && ls == 1); break;
    case IpmHold::Searched: CHECK(ds == 0 && sh == 0 && ls == 2); break;
  }
}

static const int DEPTH = 6;
static long sequences = 0, steps = 0;
static bool entered[5][2][5][2];   // [state][solved] entered from [state][solved]

static void walk(const IpmHold& h0, const Flags& f0, int depth) {
  for (int c = 0; c < N_CALLS; ++c) {
    IpmHold h = h0;
    Flags f = f0;
    bool first_h = false, first_f = false;
    const bool ok_h = call_hold(h, Call(c), &first_h), ok_f = call_flags(f, Call(c), &first_f);
    CHECK(ok_h == ok_f);           // accepted or refused alike
    CHECK(first_h == first_f);     // "the counts are not on the host yet" alike
    check_same(h, f);
    if (!ok_h) CHECK(h.state == h0.state && h.solved == h0.solved);
    entered[h.state][h.solved][h0.state][h0.solved] = true;
    ++steps;
    if (depth + 1 < DEPTH) walk(h, f, depth + 1);
    else ++sequences;
  }
}

int main() {
  const IpmHold fresh;
  check_same(fresh, Flags{});
  walk(fresh, Flags{}, 0);
  // the start clears `solved` and only a solve sets it, and a solve leaves Held: the three states of the hooks' pass never
  // coincide with multipliers of a solve.  Every other pair is reached, and by DEPTH from every pair a single call can reach it from.
  int pairs = 0;
  for (int s = 0; s < 5; ++s)
    for (int v = 0; v < 2; ++v) {
      bool any = false;
      for (int s0 = 0; s0 < 5; ++s0)
        for (int v0 = 0; v0 < 2; ++v0) any = any || entered[s][v][s0][v0];
      const bool hook_state = s == IpmHold::Started || s == IpmHold::Direction || s == IpmHold::Searched;
      CHECK(any == !(hook_state && v == 1));
      pairs += any;
    }
  CHECK(pairs == 7);
  // walking one call further enters nothing new: DEPTH - 1 calls already entered every pair from every predecessor
  bool before[5][2][5][2];
  for (int i = 0; i < 100; ++i) (&before[0][0][0][0])[i] = (&entered[0][0][0][0])[i];
  const long counted = sequences;
  for (int s = 0; s < 5; ++s)
    for (int v = 0; v < 2; ++v) {
      bool reached = false;
      for (int s0 = 0; s0 < 5; ++s0)
        for (int v0 = 0; v0 < 2; ++v0) reached = reached || before[s][v][s0][v0];
      if (!reached) continue;
      // (the flags of a state are the table's: check_same has held on every step above)
      IpmHold h;
      h.state = IpmHold::State(s);
      h.solved = v != 0;
      Flags f;
      f.solved = h.solved;
      f.debug_started = s == IpmHold::Started;
      f.state_held = h.holds_state();
      f.debug_ls = s == IpmHold::Direction ? 1 : (s == IpmHold::Searched ? 2 : 0);
      for (int c = 0; c < N_CALLS; ++c) {
        IpmHold h1 = h;
        Flags f1 = f;
        bool a = false, b = false;
        CHECK(call_hold(h1, Call(c), &a) == call_flags(f1, Call(c), &b) && a == b);
        check_same(h1, f1);
        CHECK(before[h1.state][h1.solved][s][v]);
      }
    }
  std::printf("ok: %ld sequences of %d calls (%d calls with their outcomes), %ld steps, %d reachable (state, solved) pairs\n", counted, DEPTH,
              int(N_CALLS), steps, pairs);
  return 0;
}
