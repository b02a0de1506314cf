// chain_signature.hpp -- a chain descriptor (knh_stage_desc[]) checked and turned into the device signature
// (kernel_registry.hpp: one character per stage, operands and signal slots for graph-shaped voices), and what a bank's init
// reads off the two: the frame-parallel interpreter's program, the envelopes' task order, whether a voice can finish.
// Included by bank.hip only.
#pragma once

namespace {

// Chain descriptor -> device signature (kernel_registry.hpp) with structural validation.
// outs (or null): the node-output stages of the two connected graph outputs (knh_bank_connect_outputs); null, or the last
// stage twice, is the voice whose one signal is the last stage's.
int build_signature(const knh_stage_desc* st, uint32_t n, std::string* sig, std::string* why, const uint32_t* outs = nullptr) {
  if (n == 0) { *why = "empty chain"; return KNH_ERR_INVALID_ARGUMENT; }
  sig->clear();
  bool have_x = false;
  // KNH_STAGE_FLAG_READER_CH1 stages: companion[r] = the stage that stands for output channel 1 of the reader stage r
  std::vector<int> companion(n, -1);
  for (uint32_t i = 0; i < n; ++i) {
    if (st[i].kind >= KNH_STAGE_KIND_COUNT || !(st[i].flags & KNH_STAGE_FLAG_READER_CH1)) continue;
    if (st[i].kind != KNH_STAGE_BUFFER_READER) { *why = "READER_CH1 is only defined for BUFFER_READER"; return KNH_ERR_INVALID_ARGUMENT; }
    if (st[i].flags != KNH_STAGE_FLAG_READER_CH1 || st[i].ar_param != 0 || st[i].input2 != 0 || st[i].delayed_changes_per_block != 0) {
      *why = "a READER_CH1 stage is the second output of a BufferReader, not a node: ar_param, input2, delayed_changes_per_block and every other flag must be 0";
      return KNH_ERR_INVALID_ARGUMENT;
    }
    if (st[i].input == 0 || st[i].input > i || st[st[i].input - 1].kind != KNH_STAGE_BUFFER_READER || (st[st[i].input - 1].flags & KNH_STAGE_FLAG_READER_CH1)) {
      *why = "a READER_CH1 stage names the BufferReader stage it is channel 1 of (input = 1 + its index, an earlier stage)";
      return KNH_ERR_INVALID_ARGUMENT;
    }
    if (companion[st[i].input - 1] >= 0) { *why = "at most one READER_CH1 stage per BufferReader"; return KNH_ERR_INVALID_ARGUMENT; }
    companion[st[i].input - 1] = static_cast<int>(i);
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (st[i].kind >= KNH_STAGE_KIND_COUNT) { *why = "unknown stage kind"; return KNH_ERR_INVALID_ARGUMENT; }
    const bool ch1 = is_reader_ch1(st[i]);
    const bool fb = is_feedback(st[i].kind, st[i].flags);  // a feedback edge: the FeedbackSource, 'x'
    if (is_wrapper_kind(st[i].kind) && i > 0) {  // the node the wrapper would wrap: a reader with two outputs?
      uint32_t k = i - 1;
      while (k > 0 && is_wrapper_kind(st[k].kind)) --k;
      if (is_reader_ch1(st[k]) || (st[k].kind == KNH_STAGE_BUFFER_READER && companion[k] >= 0)) {
        *why = "a wrapper stage on a BufferReader with a READER_CH1 companion would have to act on both channels: use a MUL_CONST (ADD_CONST, ...) per channel";
        return KNH_ERR_UNSUPPORTED_CHAIN;
      }
    }
    const bool source = !ch1 && (st[i].kind == KNH_STAGE_SIN_WT || st[i].kind == KNH_STAGE_SIN_NUMERIC || st[i].kind == KNH_STAGE_PHASOR ||
                        st[i].kind == KNH_STAGE_WHITE_NOISE || st[i].kind == KNH_STAGE_PINK_NOISE || st[i].kind == KNH_STAGE_BROWN_NOISE ||
                        st[i].kind == KNH_STAGE_RANDOM_LIN ||
                        st[i].kind == KNH_STAGE_POLYBLEP || st[i].kind == KNH_STAGE_BUFFER_READER || st[i].kind == KNH_STAGE_INPUT ||
                        is_env_source(st[i].kind, st[i].flags));
    const bool env_src = is_env_source(st[i].kind, st[i].flags);  // the envelope alone: 'b' 'j' 'l' for 'A' 'E' 'V'
    const bool ar = st[i].kind == KNH_STAGE_SIN_WT && (st[i].flags & KNH_STAGE_FLAG_AR_FREQ);
    const bool wt = st[i].kind == KNH_STAGE_SIN_WT && (st[i].flags & KNH_STAGE_FLAG_WAVETABLE);  // OscWt: 'M' for 'W', 'k' for 'R'
    const bool math2 = is_math2_kind(st[i].kind);
    if (st[i].flags & ~(KNH_STAGE_FLAG_AR_FREQ | KNH_STAGE_FLAG_SMOOTH_PARAMS | KNH_STAGE_FLAG_READER_CH1 | KNH_STAGE_FLAG_WAVETABLE | KNH_STAGE_FLAG_ENV_SOURCE | KNH_STAGE_FLAG_FEEDBACK)) { *why = "unknown stage flag"; return KNH_ERR_INVALID_ARGUMENT; }
    if (st[i].flags & KNH_STAGE_FLAG_FEEDBACK) {  // Graph::connect2_feedback: the flagged stage is the edge's FeedbackSource, `input` the node it taps
      if (st[i].kind != KNH_STAGE_INPUT) { *why = "FEEDBACK is only defined for KNH_STAGE_INPUT"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].flags != KNH_STAGE_FLAG_FEEDBACK) { *why = "a FEEDBACK stage takes no other stage flag"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].ar_param != 0 || st[i].input2 != 0 || st[i].delayed_changes_per_block != 0) {
        *why = "a FEEDBACK stage is a feedback edge, not a parameterised node: ar_param, input2 and delayed_changes_per_block must be 0";
        return KNH_ERR_INVALID_ARGUMENT;
      }
      if (st[i].input == 0) { *why = "a FEEDBACK stage names the stage whose output it delays by one block (input = 1 + its index)"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].input > n) { *why = "a FEEDBACK stage names a stage of this voice: input is beyond the last stage"; return KNH_ERR_INVALID_ARGUMENT; }
      const knh_stage_desc& tap = st[st[i].input - 1];
      if (tap.kind >= KNH_STAGE_KIND_COUNT) { *why = "unknown stage kind"; return KNH_ERR_INVALID_ARGUMENT; }
      if (tap.kind == KNH_STAGE_INPUT) { *why = "a feedback edge starts at a node, not at a bank input or another feedback edge (put the input through `* 1.0`)"; return KNH_ERR_INVALID_ARGUMENT; }
      if (is_reader_ch1(tap)) { *why = "a feedback edge cannot start at a READER_CH1 stage (put that channel through `* 1.0`)"; return KNH_ERR_INVALID_ARGUMENT; }
      if (tap.kind == KNH_STAGE_PAN2 || tap.kind == KNH_STAGE_GALACTIC) { *why = "a feedback edge starts at a node with one output: not at Pan2 or Galactic"; return KNH_ERR_INVALID_ARGUMENT; }
    }
    if ((st[i].flags & KNH_STAGE_FLAG_ENV_SOURCE) && !is_env_kind(st[i].kind)) { *why = "ENV_SOURCE is only defined for MUL_ENV_ASR, MUL_ENV_AR and MUL_ENVELOPE"; return KNH_ERR_INVALID_ARGUMENT; }
    if ((st[i].flags & KNH_STAGE_FLAG_ENV_SOURCE) && (st[i].flags & (KNH_STAGE_FLAG_AR_FREQ | KNH_STAGE_FLAG_READER_CH1 | KNH_STAGE_FLAG_WAVETABLE))) { *why = "ENV_SOURCE cannot be combined with AR_FREQ, READER_CH1 or WAVETABLE"; return KNH_ERR_INVALID_ARGUMENT; }
    if (env_src && st[i].input != 0) { *why = "an ENV_SOURCE stage is a source: it reads no signal (input = 0)"; return KNH_ERR_INVALID_ARGUMENT; }
    if (env_src && st[i].input2 != 0 && st[i].ar_param == 0) { *why = "input2 of an ENV_SOURCE stage is the driver of an audio-rate parameter: it needs ar_param"; return KNH_ERR_INVALID_ARGUMENT; }
    if ((st[i].flags & KNH_STAGE_FLAG_WAVETABLE) && st[i].kind != KNH_STAGE_SIN_WT) { *why = "WAVETABLE is only defined for SIN_WT"; return KNH_ERR_INVALID_ARGUMENT; }
    if ((st[i].flags & KNH_STAGE_FLAG_SMOOTH_PARAMS) && (st[i].flags & KNH_STAGE_FLAG_AR_FREQ)) { *why = "SMOOTH_PARAMS and AR_FREQ cannot be combined"; return KNH_ERR_INVALID_ARGUMENT; }
    if ((st[i].flags & KNH_STAGE_FLAG_SMOOTH_PARAMS) && is_wrapper_kind(st[i].kind)) { *why = "SMOOTH_PARAMS applies to a node, not to a wrapper stage"; return KNH_ERR_INVALID_ARGUMENT; }
    if ((st[i].flags & KNH_STAGE_FLAG_AR_FREQ) && st[i].kind != KNH_STAGE_SIN_WT) { *why = "AR_FREQ is only defined for SIN_WT"; return KNH_ERR_INVALID_ARGUMENT; }
    // operands: `input` / `input2` name the stage whose output is read (1 + its index), 0 = the stage before this one
    if ((st[i].input > i && !fb) || st[i].input2 > i) { *why = "a stage reads the output of an earlier stage"; return KNH_ERR_INVALID_ARGUMENT; }
    if (math2 && (st[i].input == 0 || st[i].input2 == 0)) { *why = "a KNH_STAGE_MATH_* stage names both of its operands (input, input2)"; return KNH_ERR_INVALID_ARGUMENT; }
    if (!math2 && st[i].input2 != 0 && st[i].ar_param == 0 && st[i].kind != KNH_STAGE_GALACTIC) { *why = "input2 is the second operand of the KNH_STAGE_MATH_* stages, the driver of an audio-rate parameter (ar_param) and the right input of Galactic"; return KNH_ERR_INVALID_ARGUMENT; }
    if (math2 && st[i].ar_param != 0) { *why = "a KNH_STAGE_MATH_* stage has no parameters"; return KNH_ERR_INVALID_ARGUMENT; }
    if (is_math1_kind(st[i].kind)) {  // Math1UGen (math.rs:167-305): one operand (`input`), no parameters -- nothing an audio-rate link, WrPreciseTiming or WrSmoothParams could act on
      if (st[i].ar_param != 0 || st[i].input2 != 0) { *why = "a KNH_STAGE_MATH1_* stage has no parameters (ar_param = 0, input2 = 0)"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].delayed_changes_per_block != 0) { *why = "a KNH_STAGE_MATH1_* stage has no parameters: delayed_changes_per_block must be 0"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].flags & KNH_STAGE_FLAG_SMOOTH_PARAMS) { *why = "a KNH_STAGE_MATH1_* stage has no parameters: SMOOTH_PARAMS does not apply"; return KNH_ERR_INVALID_ARGUMENT; }
    }
    if (is_wrapper_kind(st[i].kind) && st[i].input != 0) { *why = "a wrapper stage wraps the stage before it (input = 0)"; return KNH_ERR_INVALID_ARGUMENT; }
    if (source && !ar && !fb && st[i].input != 0) { *why = "a source stage reads no signal"; return KNH_ERR_INVALID_ARGUMENT; }
    if ((!source || ar) && !have_x) { *why = "stage needs a preceding signal"; return KNH_ERR_INVALID_ARGUMENT; }
    if ((st[i].kind == KNH_STAGE_SAMPLE_DELAY || st[i].kind == KNH_STAGE_ALLPASS_DELAY || st[i].kind == KNH_STAGE_ALLPASS_FB_DELAY || fb) &&
        std::count_if(sig->begin(), sig->end(), [](char c) { return c == 'D' || c == 'Y' || c == 'Z' || c == 'x'; }) >= KNH_MAX_DELAY_STAGES) {
      // (every delay stage and every feedback edge has a ring of its own per voice; the restart kernel's arguments name each one's rings: RestartArgs)
      *why = "a voice holds at most KNH_MAX_DELAY_STAGES delay stages and feedback edges together";
      return KNH_ERR_UNSUPPORTED_CHAIN;
    }
    if (st[i].kind == KNH_STAGE_MUL_ENVELOPE && sig->find_first_of("Vl") != std::string::npos) { *why = "at most one Envelope stage per chain"; return KNH_ERR_INVALID_ARGUMENT; }
    if (st[i].kind == KNH_STAGE_PAN2 && i + 1 != n) { *why = "Pan2 ends the chain: it must be the last stage"; return KNH_ERR_INVALID_ARGUMENT; }
    if (st[i].kind == KNH_STAGE_PAN2 && st[i].delayed_changes_per_block > 0) { *why = "Pan2 cannot be wrapped in WrPreciseTiming here (its gains change at block boundaries)"; return KNH_ERR_INVALID_ARGUMENT; }
    if (st[i].kind == KNH_STAGE_GALACTIC) {  // the reverb ends a chain of its own kind (galactic_bank.hpp)
      if (i + 1 != n) { *why = "Galactic ends the chain: it must be the last stage"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].delayed_changes_per_block > 0) { *why = "Galactic cannot be wrapped in WrPreciseTiming here (its parameters take effect at the next process call)"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].ar_param != 0) { *why = "Galactic has no audio-rate parameter (ar_param = 0)"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].flags != 0) { *why = "Galactic takes no stage flags"; return KNH_ERR_INVALID_ARGUMENT; }
      // (l | r) >> Galactic: input and input2 name the stages that feed its left and right input; neither: the running signal on both
      if (st[i].input2 != 0 && st[i].input == 0) { *why = "Galactic's right input (input2) is named together with its left one (input)"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].input2 == 0 && st[i].input != 0 && st[i].input != i) { *why = "Galactic names both of its inputs (input, input2) or neither (both are the voice's running signal then)"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].input2 != 0 && (st[st[i].input - 1].kind == KNH_STAGE_INPUT || st[st[i].input2 - 1].kind == KNH_STAGE_INPUT)) {
        *why = "an input of Galactic starts at a node, not at a bank input (put the input through `* 1.0`)";
        return KNH_ERR_INVALID_ARGUMENT;
      }
      if (sig->find_first_of("DYZ") != std::string::npos) { *why = "a chain that ends in Galactic holds no other delay stage"; return KNH_ERR_INVALID_ARGUMENT; }
      if (sig->find('x') != std::string::npos) { *why = "a chain that ends in Galactic holds no feedback edge"; return KNH_ERR_UNSUPPORTED_CHAIN; }
    }
    if (st[i].ar_param != 0) {  // an audio-rate parameter: the node's float parameter ar_param - 1 is driven by the signal input2 names
      const uint32_t p = st[i].ar_param - 1u;
      if (p >= static_cast<uint32_t>(kKinds[st[i].kind].n_params) || expected_value_kind(st[i].kind, p) != KNH_VALUE_FLOAT) { *why = "ar_param names a float parameter of the stage (1 + its index)"; return KNH_ERR_INVALID_ARGUMENT; }
      if (!ar_param_supported(st[i].kind, p)) { *why = "this parameter cannot be driven at audio rate here (knh_stage_desc.ar_param lists what can)"; return KNH_ERR_UNSUPPORTED_CHAIN; }
      if (st[i].input2 == 0) { *why = "an audio-rate parameter names the signal that drives it (input2)"; return KNH_ERR_INVALID_ARGUMENT; }
      if (st[i].flags & (KNH_STAGE_FLAG_AR_FREQ | KNH_STAGE_FLAG_SMOOTH_PARAMS)) { *why = "ar_param cannot be combined with AR_FREQ or SMOOTH_PARAMS on one stage"; return KNH_ERR_INVALID_ARGUMENT; }
      if (kKinds[st[i].kind].sig == 'I' || (st[st[i].input2 - 1].kind == KNH_STAGE_INPUT && !is_feedback(KNH_STAGE_INPUT, st[st[i].input2 - 1].flags))) { *why = "an audio-rate parameter edge starts at a node, not at a bank input (put the input through `* 1.0`)"; return KNH_ERR_INVALID_ARGUMENT; }
    }
    // ('T': a reader with two outputs; '2': its second output, which is no device stage and leaves the signature below)
    sig->push_back(fb ? 'x' : env_src ? env_source_sig(st[i].kind) : wt ? (ar ? 'k' : 'M') : ar ? 'R' : ch1 ? '2' : (st[i].kind == KNH_STAGE_BUFFER_READER && companion[i] >= 0) ? 'T' : kKinds[st[i].kind].sig);
    have_x = true;
  }
  // A voice that is a graph (a stage that names its operands, a MathUGen of two signals, a second source): every stage is
  // annotated "@a,b,o" with the SIGNAL SLOTS it reads and writes -- they are part of the kernel's type (knh_dev::At).  Slots
  // are handed out like registers, a signal's slot free again after its last reader, so that a voice of a thousand stages
  // (the reference's 256-oscillator FM cascade) keeps a handful of signals alive, not a thousand.
  // (a voice with two connected outputs is a graph even when its stage list is a plain chain: two signals leave it)
  const bool connected = outs && n > 0 && !(outs[0] == n - 1 && outs[1] == n - 1);
  bool dag = connected;
  {
    uint32_t sources = 0, edges = 0, envelopes = 0;
    for (uint32_t i = 0; i < n; ++i) { edges += is_feedback(st[i].kind, st[i].flags); envelopes += is_env_kind(st[i].kind); }
    if (edges > 0 && envelopes > 1) {
      // (where the FeedbackSink stands among the tasks -- and with it which envelope's mark names the done frame -- is not pinned here)
      *why = "a voice with a feedback edge holds at most one envelope stage";
      return KNH_ERR_UNSUPPORTED_CHAIN;
    }
    dag = dag || edges > 0;  // always a graph voice
    for (uint32_t i = 0; i < n; ++i) {
      const bool ar = st[i].kind == KNH_STAGE_SIN_WT && (st[i].flags & KNH_STAGE_FLAG_AR_FREQ);
      sources += (std::strchr("WNPUKOGBFI", kKinds[st[i].kind].sig) != nullptr || is_env_source(st[i].kind, st[i].flags)) && !ar && !is_reader_ch1(st[i]);
      dag = dag || is_math2_kind(st[i].kind) || (st[i].input != 0 && st[i].input != i) || st[i].ar_param != 0 || is_reader_ch1(st[i]);
    }
    dag = dag || sources > 1;
  }
  if (dag && n > 512 && !(interp_can_run(st, n) && n <= 4096 && !connected)) {
    // every stage unrolls into the one kernel the voice is fused into: 91 stages build in 2 s, 379 in a minute, and the
    // time grows faster than the count (the reference's 256-oscillator FM cascade, 1 531 stages, does not finish)
    // (graphs of SinWt oscillators and arithmetic alone are not fused at all: up to 4 096 stages run in kernels_interp.hip)
    *why = connected ? "a voice with two connected outputs is fused like any graph: it may hold at most 512 stages"
                     : "a voice that is a graph may hold at most 512 stages (4 096 if it is made of SinWt oscillators and arithmetic only)";
    return KNH_ERR_UNSUPPORTED_CHAIN;
  }
  if (dag) {
    std::vector<int> a(n, -1), b(n, -1), last_use(n, -1);
    // "the output of stage k" is the output of the NODE stage k stands for: if wrapper stages follow it (they wrap it: the
    // reference's wr_mul() etc. are part of the UGen), what a reader gets is the last wrapper's output
    auto node_output = [&](int k) {
      while (k + 1 < static_cast<int>(n) && is_wrapper_kind(st[k + 1].kind)) ++k;
      return k;
    };
    // Feedback edges (KNH_STAGE_FLAG_FEEDBACK): edge e's source is stage fb_src[e], its tap the node output fb_tap[e].  The device
    // list has two ops per edge: 'x' fills the source's signal slot from the voice's ring, 'y' -- no host stage stands for it --
    // stores the tapped signal's slot to the ring, directly behind the tapped node's output, and passes the signal on.  Both
    // touch the same ring positions tile by tile, so their order is the edge's one-block delay: a tap LATER than the source has
    // its 'x' at the source's place (the 'y' comes later in the same tile); a tap EARLIER than the source has its 'x'
    // immediately in front of its 'y', the slot held until the source's last reader (graph_tests.rs:221-254, feedback_nodes2).
    std::vector<uint32_t> fb_src, fb_tap;
    for (uint32_t i = 0; i < n; ++i)
      if ((*sig)[i] == 'x') { fb_src.push_back(i); fb_tap.push_back(static_cast<uint32_t>(node_output(static_cast<int>(st[i].input) - 1))); }
    for (uint32_t i = 0; i < n; ++i) {
      const bool reads = i > 0 && !(std::strchr("WMNPUKOGBFIT2bjlx", (*sig)[i]) != nullptr);  // 'R' reads, the plain sources do not (nor does a reader's second output: it IS the reader)
      if (is_math2_kind(st[i].kind)) { a[i] = node_output(st[i].input - 1); b[i] = node_output(st[i].input2 - 1); }
      else if (reads) a[i] = st[i].input ? node_output(st[i].input - 1) : static_cast<int>(i) - 1;
      if (st[i].ar_param != 0) b[i] = node_output(st[i].input2 - 1);  // the signal that drives the parameter
      if (a[i] >= 0) last_use[a[i]] = static_cast<int>(i);
      if (b[i] >= 0) last_use[b[i]] = static_cast<int>(i);
    }
    last_use[n - 1] = static_cast<int>(n);  // the voice's output
    if (connected) {  // ... or the two connected ones: neither slot is given to a later stage
      last_use[n - 1] = -1;
      last_use[outs[0]] = last_use[outs[1]] = static_cast<int>(n);
    }
    std::vector<int> slot(n, -1);
    std::vector<char> busy;
    std::string out;
    auto num = [](int v) { return v < 0 ? std::string("_") : std::to_string(v); };  // "_": none
    int last_o = -1;  // the slot the last device op writes: the voice's signal unless the list's end says otherwise
    for (uint32_t i = 0; i < n; ++i) {
      if ((*sig)[i] == '2') continue;  // a reader's second output: its slot was handed out with the reader's, it is no device stage
      if ((*sig)[i] == 'x' && slot[i] >= 0) continue;  // a feedback source behind its tap: its 'x' stands in front of the edge's 'y'
      const int sa = a[i] >= 0 ? slot[a[i]] : -1, sb = b[i] >= 0 ? slot[b[i]] : -1;
      // operands whose last reader this is give their slot back first: the stage may then write where it read
      if (a[i] >= 0 && last_use[a[i]] == static_cast<int>(i)) busy[sa] = 0;
      if (b[i] >= 0 && last_use[b[i]] == static_cast<int>(i) && sb >= 0) busy[sb] = 0;
      int o = -1;
      if (sa >= 0 && !busy[sa] && !is_math2_kind(st[i].kind)) o = sa;  // in place, like a chain
      for (size_t k = 0; o < 0 && k < busy.size(); ++k)
        if (!busy[k]) o = static_cast<int>(k);
      if (o < 0) { o = static_cast<int>(busy.size()); busy.push_back(0); }
      if (last_use[i] >= 0) busy[o] = 1;  // (a signal nobody reads holds its slot only while it is written)
      slot[i] = o;
      int o2 = -1;
      if (companion[i] >= 0) {  // a reader with two outputs writes both slots every frame: the second one is another slot, held like the first until its last reader
        for (size_t k = 0; o2 < 0 && k < busy.size(); ++k)
          if (!busy[k] && static_cast<int>(k) != o) o2 = static_cast<int>(k);
        if (o2 < 0) { o2 = static_cast<int>(busy.size()); busy.push_back(0); }
        if (last_use[companion[i]] >= 0) busy[o2] = 1;
        slot[companion[i]] = o2;
      }
      out.push_back((*sig)[i]);
      if (st[i].ar_param != 0) out += "%" + std::to_string(st[i].ar_param - 1);  // "%P": parameter P at audio rate (knh_dev::ArP)
      if ((*sig)[i] == 'x') out += "$" + std::to_string(std::find(fb_src.begin(), fb_src.end(), i) - fb_src.begin());  // "$E": edge E's ring (knh_dev::FbRead<E>)
      out += "@" + num(sa) + "," + num(sb) + "," + num(o);
      if (o2 >= 0) out += "," + num(o2);  // "@a,b,o,o2": the slot of the node's second output (knh_dev::At2)
      last_o = o;
      for (size_t e = 0; e < fb_src.size(); ++e) {  // the edges that tap this node's output
        if (fb_tap[e] != i) continue;
        const int s_tap = slot[i];
        if (fb_src[e] > i) {  // the source comes later: last block's samples leave the ring before this block's go in
          const char was = busy[s_tap];
          busy[s_tap] = 1;  // (a tapped signal nobody else reads still holds its slot until the 'y' behind it)
          int r = -1;
          for (size_t k = 0; r < 0 && k < busy.size(); ++k)
            if (!busy[k]) r = static_cast<int>(k);
          if (r < 0) { r = static_cast<int>(busy.size()); busy.push_back(0); }
          busy[s_tap] = was;
          if (last_use[fb_src[e]] >= 0) busy[r] = 1;
          slot[fb_src[e]] = r;
          out += "x$" + std::to_string(e) + "@_,_," + num(r);
        }
        out += "y$" + std::to_string(e) + "@" + num(s_tap) + ",_," + num(s_tap);  // (in place: the tapped signal goes on as it is)
        last_o = s_tap;
      }
    }
    *sig = out + "#" + std::to_string(busy.size());  // "#R": the number of slots
    if (!connected && !(st[n - 1].flags & KNH_STAGE_FLAG_READER_CH1) && last_o != slot[n - 1]) *sig += "=" + std::to_string(slot[n - 1]);  // (the voice's signal is not the last device op's: a feedback source whose 'x' stands earlier)
    if (!connected && (st[n - 1].flags & KNH_STAGE_FLAG_READER_CH1)) *sig += "=" + std::to_string(slot[n - 1]);  // "#R=k": the voice's signal is a reader's second output, in slot k (knh_dev::Out1)
    if (connected) *sig += ":" + std::to_string(slot[outs[0]]) + "," + std::to_string(slot[outs[1]]);  // "#R:l,r": the slots of the two connected outputs
  }
  return KNH_OK;
}

// A chain that ends in KNH_STAGE_GALACTIC (checked by build_signature): the node-output stages, in the chain before the
// reverb, of the signals on its left and right input.  False: the mono spelling, both inputs are the last stage's signal.
inline bool galactic_inputs(const knh_stage_desc* st, uint32_t n, uint32_t outs[2]) {
  const knh_stage_desc& g = st[n - 1];
  outs[0] = outs[1] = n - 2;
  if (g.input2 == 0) return false;
  const uint32_t op[2] = {g.input, g.input2};
  for (int c = 0; c < 2; ++c) {
    outs[c] = op[c] - 1u;
    while (outs[c] + 1 < n - 1 && is_wrapper_kind(st[outs[c] + 1].kind)) ++outs[c];
  }
  return !(outs[0] == n - 2 && outs[1] == n - 2);
}

// The signature of a voice made of SinWt oscillators and arithmetic alone, Math1UGen's functions included (interp_can_run) -> the program of the
// frame-parallel interpreter (kernels_interp.hip), one op per stage; *n_sigs its signal slots, *out the slot of the voice's
// output.  False: the signature is malformed.
bool parse_frame_program(const std::string& signature, const std::vector<StageInfo>& stages, std::vector<knh_dev::InterpOp>* prog, unsigned* n_sigs, unsigned* out) {
  const bool graph = signature_is_dag(signature);
  prog->clear();
  size_t si = 0;
  const char* p = signature.c_str();
  while (*p && *p != '#') {
    knh_dev::InterpOp op{};
    const char c = *p++;
    int v[3] = {-1, -1, -1};
    if (*p == '@') {
      ++p;
      for (int k = 0; k < 3; ++k) {
        if (*p == '_') { ++p; } else { v[k] = 0; while (*p >= '0' && *p <= '9') v[k] = v[k] * 10 + (*p++ - '0'); }
        if (*p == ',') ++p;
      }
    }
    switch (c) {
      case 'W': op.kind = knh_dev::INTERP_SIN_WT; break;
      case 'm': op.kind = knh_dev::INTERP_VAL_MUL; break;
      case 'a': op.kind = knh_dev::INTERP_VAL_ADD; break;
      case 's': op.kind = knh_dev::INTERP_VAL_SUB; break;
      case 'd': op.kind = knh_dev::INTERP_VAL_DIV; break;
      case 'v': op.kind = knh_dev::INTERP_VAL_VSUB; break;
      case 'q': op.kind = knh_dev::INTERP_VAL_VDIV; break;
      case '*': op.kind = knh_dev::INTERP_MATH_MUL; break;
      case '+': op.kind = knh_dev::INTERP_MATH_ADD; break;
      case '-': op.kind = knh_dev::INTERP_MATH_SUB; break;
      case 'c': op.kind = knh_dev::INTERP_MATH1_CEIL; break;
      case 'r': op.kind = knh_dev::INTERP_MATH1_SQRT; break;
      case 'f': op.kind = knh_dev::INTERP_MATH1_FLOOR; break;
      case 't': op.kind = knh_dev::INTERP_MATH1_TRUNC; break;
      case 'w': op.kind = knh_dev::INTERP_MATH1_FRACT; break;
      case 'e': op.kind = knh_dev::INTERP_MATH1_EXP; break;
      default: op.kind = knh_dev::INTERP_MATH_DIV; break;
    }
    if (!graph) {  // a plain chain: one signal, every stage works on it in place
      v[0] = c == 'W' ? -1 : 0;
      v[2] = 0;
    }
    if (si >= stages.size() || v[2] < 0 || (c != 'W' && v[0] < 0)) return false;
    op.a = static_cast<unsigned short>(v[0] < 0 ? 0 : v[0]);
    op.b = static_cast<unsigned short>(v[1] < 0 ? 0 : v[1]);
    op.o = static_cast<unsigned short>(v[2]);
    op.slot = static_cast<uint32_t>(stages[si].slot_base);
    prog->push_back(op);
    ++si;
  }
  *n_sigs = *p == '#' ? static_cast<unsigned>(std::atoi(p + 1)) : (graph ? 0u : 1u);
  *out = prog->empty() ? 0u : prog->back().o;
  return si == stages.size() && *n_sigs != 0;
}

// VoiceKernelArgs::env_ranks of a voice that is a graph with several envelope stages: which envelope's mark_done names the
// voice's done frame when several finish in one block -- the last one in the reference's TASK order (graph_gen.rs:196-200),
// which for a graph is the order Graph::calculate_node_order sorts the nodes into (graph.rs:1938-2067): depth first from
// the output, a node's inputs in channel order, each node after everything it reads; nodes the output does not depend on
// come last, in the order they were pushed.  0: list order (every chain; and graphs whose task order agrees with it).
// outs (or null): the two connected outputs' stages (knh_bank_connect_outputs).  For each output edge, in channel order, the
// reference pushes the DEEPEST output node its source leads to -- get_deepest_output_node, graph.rs:1984-2018: from the
// source forward along the first node (in push order) that reads the current one through an input edge, until a node
// already pushed or one nobody reads; the last output node met on the way, the source itself if none -- and only if that
// node is not pushed yet (graph.rs:2022-2040).  The search then works from the top of that stack and never enters a node
// that is on it: as a rule the right output's subtree is ordered first, then what only the left one reads; an output
// that feeds the other one along that walk is not a root of its own, the search reaches it from the other.  Unconnected
// nodes come last, in push order.
uint64_t envelope_task_ranks(const std::string& signature, const std::vector<StageInfo>& stages, const uint32_t* outs = nullptr) {
  if (!signature_is_dag(signature)) return 0;
  const int n = static_cast<int>(stages.size());
  auto is_src = [&](int i) { return (std::strchr("WNPUKOGBFI", kKinds[stages[i].kind].sig) != nullptr || stages[i].env_source()) && !(stages[i].flags & KNH_STAGE_FLAG_AR_FREQ); };
  auto node_output = [&](int k) { while (k + 1 < n && is_wrapper_kind(stages[k + 1].kind)) ++k; return k; };
  std::vector<int> a(n, -1), b(n, -1);
  for (int i = 0; i < n; ++i) {
    if (is_math2_kind(stages[i].kind)) { a[i] = node_output(stages[i].input - 1); b[i] = node_output(stages[i].input2 - 1); }
    else if (i > 0 && !is_src(i)) a[i] = stages[i].input ? node_output(stages[i].input - 1) : i - 1;
    // an audio-rate parameter edge: followed after the node's input edges (graph.rs:1938-1980)
    if (stages[i].ar_param && !is_math2_kind(stages[i].kind)) b[i] = node_output(stages[i].input2 - 1);
  }
  // a reader's second output (KNH_STAGE_FLAG_READER_CH1) is the reader NODE: whoever reads it reads that node
  auto node_of = [&](int k) { return k >= 0 && stages[k].ch1() ? static_cast<int>(stages[k].input) - 1 : k; };
  for (int i = 0; i < n; ++i) {
    if (stages[i].ch1()) { a[i] = b[i] = -1; continue; }
    a[i] = node_of(a[i]);
    b[i] = node_of(b[i]);
  }
  uint32_t out_nodes[2] = {0, 0};
  if (outs) {
    for (int c = 0; c < 2; ++c) out_nodes[c] = static_cast<uint32_t>(node_of(static_cast<int>(outs[c])));
    outs = out_nodes;
  }
  std::vector<int> order, state(n, 0), stack{node_of(n - 1)};
  std::vector<char> root(n, 0);  // pushed as the start of the search ("visited" from then on: the search does not enter it from a reader)
  if (outs) {
    stack.clear();
    auto first_reader = [&](int k) {  // input edges only: a parameter edge is not followed forward
      for (int i = k + 1; i < n; ++i)
        if (a[i] == k || (is_math2_kind(stages[i].kind) && b[i] == k)) return i;
      return -1;
    };
    for (int c = 0; c < 2; ++c) {
      int cur = static_cast<int>(outs[c]), deepest = cur;
      while (!root[cur]) {
        const int next = first_reader(cur);
        if (next < 0) break;
        cur = next;
        if (cur == static_cast<int>(outs[0]) || cur == static_cast<int>(outs[1])) deepest = cur;
      }
      if (!root[deepest]) { stack.push_back(deepest); root[deepest] = 1; }
    }
  }
  while (!stack.empty()) {  // post-order, first operand first
    const int k = stack.back();
    if (state[k] == 0) { state[k] = 1; if (a[k] >= 0 && state[a[k]] == 0 && !root[a[k]]) { stack.push_back(a[k]); continue; } }
    if (state[k] == 1) { state[k] = 2; if (b[k] >= 0 && state[b[k]] == 0 && !root[b[k]]) { stack.push_back(b[k]); continue; } }
    if (state[k] == 2) { state[k] = 3; order.push_back(k); }
    stack.pop_back();
  }
  for (int i = 0; i < n; ++i) if (state[i] == 0) order.push_back(i);
  std::vector<int> rank(n, 0);
  for (size_t r = 0; r < order.size(); ++r) rank[order[r]] = static_cast<int>(r);
  std::vector<int> envs;
  for (int i = 0; i < n; ++i)
    if (stages[i].kind == KNH_STAGE_MUL_ENV_ASR || stages[i].kind == KNH_STAGE_MUL_ENV_AR || stages[i].kind == KNH_STAGE_MUL_ENVELOPE) envs.push_back(i);
  bool in_list_order = true;
  for (size_t j = 1; j < envs.size(); ++j) in_list_order = in_list_order && rank[envs[j - 1]] < rank[envs[j]];
  uint64_t ranks = 0;
  if (!in_list_order && envs.size() <= 15) {
    std::vector<int> by_rank(envs);
    std::sort(by_rank.begin(), by_rank.end(), [&](int x, int y) { return rank[x] < rank[y]; });
    for (size_t j = 0; j < envs.size(); ++j) {
      const uint64_t place = 1 + static_cast<uint64_t>(std::find(by_rank.begin(), by_rank.end(), envs[j]) - by_rank.begin());
      ranks |= place << (4 * j);
    }
  }
  return ranks;
}

// The chain has a stage that can end a voice: without one ALL_DONE is never reported (a chain without an envelope never finishes).
// ALL_DONE describes silence: an envelope that is a source (KNH_STAGE_FLAG_ENV_SOURCE) silences nothing and does not count.
bool chain_can_finish(const std::vector<StageInfo>& stages) {
  for (const StageInfo& st : stages)
    if ((is_env_kind(st.kind) && !st.env_source()) || st.kind == KNH_STAGE_BUFFER_READER) return true;
  return false;
}
// A block's done / running voice counts -> the flags of knh_bank_process_block.
inline uint32_t done_flags(uint32_t n_done, uint32_t n_running, bool can_finish) {
  return (n_done ? KNH_FLAG_ANY_DONE : 0u) | (can_finish && n_running == 0 ? KNH_FLAG_ALL_DONE : 0u);
}

}  // namespace
