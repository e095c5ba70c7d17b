// mioc_ode_rtc.cpp -- user-defined ODE objectives (the reference's extension point, AbstractODEObjective with the
// hooks F!, Fy!, Fu!, G, Gy!, Gu!: julia_opt/ODEObjective.jl:243-248) compiled at run time for gfx950.  Host code only:
// the kernel text is in mioc_ode_skeleton.h.
//
// mioc_ode_program_create* describe a program (ProgramSpec, validate), wrap the caller's hooks (HIP source text, the
// contract is in include/mioc.h) in that kernel text (assemble) and compile the result with hiprtc (compile);
// mioc_ode_program_source stops after assemble and hands the text out.  mioc_ode_program_eval_device loads the code
// object on the context's device at first use and launches it.  hiprtc is loaded lazily (dlopen at the first create),
// so libmioc.so carries no link-time dependency on it and loads as before where it is absent.
//
// The assembled text: the head's #defines (NY, NX, NP; NS, the stage count, for Heun / RK4 or TH, theta, for the
// implicit schemes; ND, MIOC_TERMINAL, MIOC_STATES, MIOC_SCEN, MIOC_SCEN_DATA, MIOC_SENS and MIOC_DERIVE_* only when
// asked for),
// the dual type kAdPrelude
// (derive != 0), the caller's text, the generated hooks kAdHooks (derive != 0), then kSkeletonHead and the integrator's
// body: kBodyEuler, kBodyRK (Heun, RK4) or kBodyTheta (backward Euler, implicit midpoint).  A program that does not ask
// for a feature gets no byte of it in the head, and the skeleton preprocesses to the tokens it has without it.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "mioc_internal.h"
#include "mioc_ode_skeleton.h"

namespace {

using namespace mioc_kernel_text;

constexpr int kMaxNY = 8, kMaxNX = 8, kMaxNP = 32, kMaxND = 16, kMaxSubsteps = 64, kMaxFp = 64;
constexpr size_t kMaxSource = 1u << 20;
const char *const kKernelName = "mioc_ode_program_kernel";
const char *const kNoinlineNote =
    "mioc_ad: with the generated hooks inlined the kernel needs more than 256 VGPRs; they are compiled as functions\n";

// ---- hiprtc, loaded at the first mioc_ode_program_create -------------------------------------------------------
struct Rtc {
  bool ok = false;
  std::string why;
  decltype(&hiprtcCreateProgram) create = nullptr;
  decltype(&hiprtcCompileProgram) compile = nullptr;
  decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
  decltype(&hiprtcGetProgramLog) log = nullptr;
  decltype(&hiprtcGetCodeSize) code_size = nullptr;
  decltype(&hiprtcGetCode) code = nullptr;
  decltype(&hiprtcDestroyProgram) destroy = nullptr;
};

const Rtc &rtc() {
  static const Rtc r = [] {
    Rtc q;
    void *h = nullptr;
    for (const char *name : {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"}) {
      h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (h) break;
    }
    if (!h) {
      q.why = "libhiprtc.so not found (it is part of the ROCm install)";
      return q;
    }
    q.create = reinterpret_cast<decltype(q.create)>(dlsym(h, "hiprtcCreateProgram"));
    q.compile = reinterpret_cast<decltype(q.compile)>(dlsym(h, "hiprtcCompileProgram"));
    q.log_size = reinterpret_cast<decltype(q.log_size)>(dlsym(h, "hiprtcGetProgramLogSize"));
    q.log = reinterpret_cast<decltype(q.log)>(dlsym(h, "hiprtcGetProgramLog"));
    q.code_size = reinterpret_cast<decltype(q.code_size)>(dlsym(h, "hiprtcGetCodeSize"));
    q.code = reinterpret_cast<decltype(q.code)>(dlsym(h, "hiprtcGetCode"));
    q.destroy = reinterpret_cast<decltype(q.destroy)>(dlsym(h, "hiprtcDestroyProgram"));
    q.ok = q.create && q.compile && q.log_size && q.log && q.code_size && q.code && q.destroy;
    if (!q.ok) q.why = "libhiprtc.so lacks a hiprtc entry point";
    return q;
  }();
  return r;
}

void put_log(char *log, int64_t cap, const char *text, size_t n) {
  if (!log || cap < 1) return;
  const size_t m = n < (size_t)(cap - 1) ? n : (size_t)(cap - 1);
  std::memcpy(log, text, m);
  log[m] = '\0';
}

int fail(mioc_ctx *ctx, int code, const std::string &msg) {
  ctx->err = msg;
  return code;
}

// The number after `key` in the compiler's resource remarks of the kernel (-Rpass-analysis=kernel-resource-usage), -1
// if there is none.
long remark_value(const std::string &log, const char *key) {
  size_t at = log.find(std::string("Function Name: ") + kKernelName);
  if (at == std::string::npos) return -1;
  at = log.find(key, at);
  if (at == std::string::npos) return -1;
  return std::strtol(log.c_str() + at + std::strlen(key), nullptr, 10);
}

// Does the kernel need more than the 256 architectural VGPRs (AGPRs as spill space, or vector spills to scratch)?
bool over_vgpr_file(const std::string &log) {
  return remark_value(log, " AGPRs: ") > 0 || remark_value(log, " VGPRs Spill: ") > 0;
}

// The log without the remarks.  A diagnostic is its head line ("file:line:col: kind: ...") and the indented source lines
// under it; a note belongs to the diagnostic before it.  So a clean compile leaves an empty log as before.
std::string without_remarks(const std::string &log) {
  std::string out;
  bool drop = false;
  for (size_t at = 0; at < log.size();) {
    size_t end = log.find('\n', at);
    end = end == std::string::npos ? log.size() : end + 1;
    const std::string line = log.substr(at, end - at);
    if (line[0] != ' ' && line[0] != '\n' && line.find(": note: ") == std::string::npos)
      drop = line.find(": remark: ") != std::string::npos;
    if (!drop) out += line;
    at = end;
  }
  return out;
}

}  // namespace

struct mioc_ode_program {
  int ny = 0, nx = 0, np = 0, nd = 0, flags = 0, scen = 0, sens = 0;
  int integrator = MIOC_ODE_INT_EULER, substeps = 1;
  std::vector<char> code;  // the gfx950 code object
  struct Loaded {
    int device;
    hipModule_t mod;
    hipFunction_t fn;
  };
  std::mutex mu;
  std::vector<Loaded> loaded;  // one module per device the program ran on
};

namespace {

// What a program is compiled from, besides the caller's text.
struct ProgramSpec {
  int ny, nx, np, nd, integrator, substeps, derive, flags, scen, sens;
  bool euler() const { return integrator == MIOC_ODE_INT_EULER; }
  bool implicit() const { return integrator == MIOC_ODE_INT_BEULER || integrator == MIOC_ODE_INT_MIDPOINT; }
};

// The argument checks of every create entry (include/mioc.h lists them); *len: the length of the caller's text.
int validate(const ProgramSpec &s, const char *hooks, size_t *len) {
  if (!hooks || s.ny < 1 || s.ny > kMaxNY || s.nx < 1 || s.nx > kMaxNX || s.np < 0 || s.np > kMaxNP) return MIOC_EINVAL;
  if (s.nd < 0 || s.nd > kMaxND || (s.flags & ~(MIOC_ODE_TERMINAL | MIOC_ODE_STATES))) return MIOC_EINVAL;
  if (!s.euler() && s.integrator != MIOC_ODE_INT_HEUN && s.integrator != MIOC_ODE_INT_RK4 && !s.implicit())
    return MIOC_EINVAL;
  if (s.substeps < 1 || s.substeps > kMaxSubsteps || (s.euler() && s.substeps != 1)) return MIOC_EINVAL;
  constexpr int kDeriveP = MIOC_ODE_DERIVE_FP | MIOC_ODE_DERIVE_GP | MIOC_ODE_DERIVE_EP;
  if (s.derive & ~(MIOC_ODE_DERIVE_ALL | MIOC_ODE_DERIVE_EY | kDeriveP)) return MIOC_EINVAL;
  if ((s.derive & (MIOC_ODE_DERIVE_EY | MIOC_ODE_DERIVE_EP)) && !(s.flags & MIOC_ODE_TERMINAL)) return MIOC_EINVAL;
  // sensitivities: not for the reference's Euler scheme; fp[NY][NP] lives in registers
  if ((s.sens & ~(MIOC_ODE_SENS_P | MIOC_ODE_SENS_Y0)) || (s.sens && s.euler())) return MIOC_EINVAL;
  if ((s.sens & MIOC_ODE_SENS_P) && (s.np == 0 || s.ny * s.np > kMaxFp)) return MIOC_EINVAL;
  if ((s.derive & kDeriveP) && !(s.sens & MIOC_ODE_SENS_P)) return MIOC_EINVAL;
  // per-scenario data need per-scenario state0 and parameters, and data
  if ((s.scen & ~(MIOC_ODE_SCEN | MIOC_ODE_SCEN_DATA)) || s.scen == MIOC_ODE_SCEN_DATA) return MIOC_EINVAL;
  if ((s.scen & MIOC_ODE_SCEN_DATA) && s.nd == 0) return MIOC_EINVAL;
  *len = strnlen(hooks, kMaxSource + 1);
  return *len > kMaxSource ? MIOC_EINVAL : MIOC_OK;
}

// The text handed to hiprtc, in the order include/mioc.h documents.  noinline: the head of the second compile.
std::string assemble(const ProgramSpec &s, const char *hooks, size_t len, bool noinline) {
  const char *const body = s.euler() ? kBodyEuler : s.implicit() ? kBodyTheta : kBodyRK;
  std::string src;
  src.reserve(len + std::strlen(kSkeletonHead) + std::strlen(body) +
              (s.derive ? std::strlen(kAdPrelude) + std::strlen(kAdHooks) : 0) + 1024);
  const auto define = [&src](const char *name, const std::string &value) {
    src += std::string("#define ") + name + " " + value + "\n";
  };
  if (noinline) define("MIOC_AD_NOINLINE", "1");
  define("NY", std::to_string(s.ny));
  define("NX", std::to_string(s.nx));
  define("NP", std::to_string(s.np));
  // the reference scheme's head ends here; NS: the stage count, which selects the tableau; TH: theta, 1 for backward
  // Euler and 1/2 for the implicit midpoint rule
  if (s.implicit())
    define("TH", s.integrator == MIOC_ODE_INT_BEULER ? "1.0" : "0.5");
  else if (!s.euler())
    define("NS", s.integrator == MIOC_ODE_INT_HEUN ? "2" : "4");
  // sampled data, the terminal cost and the state output are compiled in only when asked for: none adds a byte here
  if (s.nd > 0) define("ND", std::to_string(s.nd));
  if (s.flags & MIOC_ODE_TERMINAL) define("MIOC_TERMINAL", "1");
  if (s.flags & MIOC_ODE_STATES) define("MIOC_STATES", "1");
  if (s.scen & MIOC_ODE_SCEN) define("MIOC_SCEN", "1");
  if (s.scen & MIOC_ODE_SCEN_DATA) define("MIOC_SCEN_DATA", "1");
  if (s.sens) define("MIOC_SENS", std::to_string(s.sens));
  if (s.derive) {  // the guard macros and the dual type in front of the caller's text; derive == 0 adds no byte
    if (s.derive & MIOC_ODE_DERIVE_FY) define("MIOC_DERIVE_FY", "1");
    if (s.derive & MIOC_ODE_DERIVE_FU) define("MIOC_DERIVE_FU", "1");
    if (s.derive & MIOC_ODE_DERIVE_GY) define("MIOC_DERIVE_GY", "1");
    if (s.derive & MIOC_ODE_DERIVE_GU) define("MIOC_DERIVE_GU", "1");
    if (s.derive & MIOC_ODE_DERIVE_EY) define("MIOC_DERIVE_EY", "1");
    if (s.derive & MIOC_ODE_DERIVE_FP) define("MIOC_DERIVE_FP", "1");
    if (s.derive & MIOC_ODE_DERIVE_GP) define("MIOC_DERIVE_GP", "1");
    if (s.derive & MIOC_ODE_DERIVE_EP) define("MIOC_DERIVE_EP", "1");
    src += "#line 1 \"mioc_ad\"";
    src += kAdPrelude;
  }
  src += "#line 1 \"hooks\"\n";
  src.append(hooks, len);
  if (s.flags & MIOC_ODE_TERMINAL)  // still under "hooks": a text without E is diagnosed there (hooks:N) first
    src += "\n__device__ inline double mioc_terminal_needs_E(const double *p, double t, const double *y) "
           "{ return E(p, t, y); }";
  if (s.derive) {  // the generated hooks between the caller's text and the skeleton
    src += "\n#line 1 \"mioc_ad_hooks\"";
    src += kAdHooks;
  }
  src += "\n#line 1 \"mioc_ode_program_skeleton\"";
  src += kSkeletonHead;
  src += body;
  return src;
}

// One hiprtc compile of src into *code, the compiler's log behind `note` into `log`.  want_remarks: the compiler also
// reports the kernel's registers (remarks, taken out of the log again); with over_vgprs given, a kernel that needs more
// than the 256 architectural VGPRs sets it and leaves *code empty.
int compile(const std::string &src, bool want_remarks, const char *note, std::vector<char> *code, bool *over_vgprs,
            char *log, int64_t log_cap) {
  // the flags of csrc/Makefile that bear on the arithmetic: no FMA contraction, no fast-math
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math",
                        "-Rpass-analysis=kernel-resource-usage"};
  const Rtc &R = rtc();
  hiprtcProgram prog = nullptr;
  if (R.create(&prog, src.c_str(), "mioc_ode_program.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
    const char msg[] = "hiprtcCreateProgram failed";
    put_log(log, log_cap, msg, sizeof msg - 1);
    return MIOC_ECOMPILE;
  }
  const hiprtcResult rc = R.compile(prog, want_remarks ? 5 : 4, opts);
  int ret = rc == HIPRTC_SUCCESS ? MIOC_OK : MIOC_ECOMPILE;
  bool over = false;
  try {
    size_t ln = 0, cn = 0;
    std::string text;
    if (R.log_size(prog, &ln) == HIPRTC_SUCCESS && ln > 1) {
      std::vector<char> buf(ln + 1, '\0');
      if (R.log(prog, buf.data()) == HIPRTC_SUCCESS) text.assign(buf.data(), strnlen(buf.data(), ln));
    }
    if (want_remarks) {
      over = over_vgprs && ret == MIOC_OK && over_vgpr_file(text);
      text = without_remarks(text);
      text.insert(0, note);
    }
    put_log(log, log_cap, text.c_str(), text.size());
    if (ret == MIOC_OK && !over) {
      if (R.code_size(prog, &cn) != HIPRTC_SUCCESS || cn == 0) {
        ret = MIOC_ECOMPILE;
      } else {
        code->resize(cn);
        if (R.code(prog, code->data()) != HIPRTC_SUCCESS) ret = MIOC_ECOMPILE;
      }
    }
  } catch (const std::bad_alloc &) {
    ret = MIOC_ENOMEM;
    over = false;
  }
  if (over_vgprs) *over_vgprs = over;
  R.destroy(&prog);
  return ret;
}

}  // namespace

extern "C" {

int32_t mioc_ode_program_create(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, mioc_ode_program **out,
                                char *log, int64_t log_cap) {
  return mioc_ode_program_create_ex(hooks, ny, nx, nparams, MIOC_ODE_INT_EULER, 1, out, log, log_cap);
}

int32_t mioc_ode_program_create_ex(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t integrator,
                                   int32_t substeps, mioc_ode_program **out, char *log, int64_t log_cap) {
  return mioc_ode_program_create_ad(hooks, ny, nx, nparams, integrator, substeps, 0, out, log, log_cap);
}

int32_t mioc_ode_program_create_ad(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t integrator,
                                   int32_t substeps, int32_t derive, mioc_ode_program **out, char *log,
                                   int64_t log_cap) {
  return mioc_ode_program_create_bolza(hooks, ny, nx, nparams, 0, integrator, substeps, derive, 0, out, log, log_cap);
}

int32_t mioc_ode_program_create_bolza(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                      int32_t integrator, int32_t substeps, int32_t derive, int32_t flags,
                                      mioc_ode_program **out, char *log, int64_t log_cap) {
  return mioc_ode_program_create_scen(hooks, ny, nx, nparams, ndata, integrator, substeps, derive, flags, 0, out, log,
                                      log_cap);
}

int32_t mioc_ode_program_create_scen(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                     int32_t integrator, int32_t substeps, int32_t derive, int32_t flags, int32_t scen,
                                     mioc_ode_program **out, char *log, int64_t log_cap) {
  return mioc_ode_program_create_sens(hooks, ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen, 0, out,
                                      log, log_cap);
}

int32_t mioc_ode_program_create_sens(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                     int32_t integrator, int32_t substeps, int32_t derive, int32_t flags, int32_t scen,
                                     int32_t sens, mioc_ode_program **out, char *log, int64_t log_cap) {
  put_log(log, log_cap, "", 0);
  if (!out) return MIOC_EINVAL;
  *out = nullptr;
  const ProgramSpec spec{ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen, sens};
  size_t len = 0;
  if (validate(spec, hooks, &len) != MIOC_OK) return MIOC_EINVAL;
  const Rtc &R = rtc();
  if (!R.ok) {
    put_log(log, log_cap, R.why.c_str(), R.why.size());
    return MIOC_EHIP;
  }
  // With derived hooks a kernel that needs more than the 256 architectural VGPRs with every generated hook inlined at
  // each of its call sites is compiled a second time with the generated hooks as functions (MIOC_AD_NOINLINE), one body
  // each however many stages call it.
  try {
    std::unique_ptr<mioc_ode_program> p(new mioc_ode_program);
    p->ny = ny, p->nx = nx, p->np = nparams, p->nd = ndata, p->flags = flags, p->scen = scen, p->sens = sens;
    p->integrator = integrator, p->substeps = substeps;
    bool over = false;
    int ret = compile(assemble(spec, hooks, len, false), derive != 0, "", &p->code, &over, log, log_cap);
    if (ret == MIOC_OK && over)
      ret = compile(assemble(spec, hooks, len, true), true, kNoinlineNote, &p->code, nullptr, log, log_cap);
    if (ret == MIOC_OK) *out = p.release();
    return ret;
  } catch (const std::bad_alloc &) {
    return MIOC_ENOMEM;
  }
}

int64_t mioc_ode_program_source(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                int32_t integrator, int32_t substeps, int32_t derive, int32_t flags, int32_t noinline,
                                char *text, int64_t text_cap) {
  return mioc_ode_program_source_scen(hooks, ny, nx, nparams, ndata, integrator, substeps, derive, flags, 0, noinline,
                                      text, text_cap);
}

int64_t mioc_ode_program_source_scen(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                     int32_t integrator, int32_t substeps, int32_t derive, int32_t flags, int32_t scen,
                                     int32_t noinline, char *text, int64_t text_cap) {
  return mioc_ode_program_source_sens(hooks, ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen, 0,
                                      noinline, text, text_cap);
}

int64_t mioc_ode_program_source_sens(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                     int32_t integrator, int32_t substeps, int32_t derive, int32_t flags, int32_t scen,
                                     int32_t sens, int32_t noinline, char *text, int64_t text_cap) {
  put_log(text, text_cap, "", 0);
  const ProgramSpec spec{ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen, sens};
  size_t len = 0;
  if (validate(spec, hooks, &len) != MIOC_OK) return MIOC_EINVAL;
  try {
    const std::string src = assemble(spec, hooks, len, noinline != 0);
    put_log(text, text_cap, src.c_str(), src.size());
    return (int64_t)src.size();
  } catch (const std::bad_alloc &) {
    return MIOC_ENOMEM;
  }
}

int32_t mioc_ode_program_destroy(mioc_ode_program *prog) {
  if (!prog) return MIOC_EINVAL;
  int rc = MIOC_OK;
  if (!prog->loaded.empty()) {
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    for (const auto &l : prog->loaded) {  // a launch may still be in flight on this device
      if (hipSetDevice(l.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
          hipModuleUnload(l.mod) != hipSuccess)
        rc = MIOC_EHIP;
    }
    if (have_prev) (void)hipSetDevice(prev);
  }
  delete prog;
  return rc;
}

// The body of every eval entry.  nu = 0: every control is the DP's (mioc_ode_program_eval_device); nu >= 1: the first
// nu controls are continuous and the levels describe the other nx - nu (mioc_ode_program_eval_mixed_device).  S = 0:
// state0 and params are host arrays, passed by value to a program without scenarios; S >= 1: they are the device
// arrays of S scenarios for a program compiled with them (mioc_ode_program_eval_scen_device).  d_Jp, d_Jy0: the
// sensitivities of a program compiled with them (mioc_ode_program_eval_sens_device), NULL from every other entry.
static int32_t program_eval(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K, const double *d_x, int64_t nt,
                            double T0, double T1, int64_t S, const double *state0, const double *params,
                            const double *d_data, double *d_J, double *d_df, double *d_Y, double *d_Jp = nullptr,
                            double *d_Jy0 = nullptr) {
  if (!ctx) return MIOC_EINVAL;
  MIOC_JOIN_BT(ctx);
  if (!prog) return fail(ctx, MIOC_EINVAL, "no ODE program");
  if (K < 1 || nt < 1 || K > INT32_MAX || nt > INT32_MAX || !d_x) return fail(ctx, MIOC_EINVAL, "bad K / nt / x");
  if (S == 0 && prog->scen)
    return fail(ctx, MIOC_EINVAL, "the program was compiled with scenarios: use mioc_ode_program_eval_scen_device");
  if (S != 0 && !prog->scen) return fail(ctx, MIOC_EINVAL, "the program was not compiled with scenarios");
  if (S < 0 || (S > 0 && K % S != 0)) return fail(ctx, MIOC_EINVAL, "need S >= 1 scenarios and K a multiple of S");
  if (!state0 || (prog->np > 0 && !params)) return fail(ctx, MIOC_EINVAL, "state0 / params missing");
  if (!(T1 > T0)) return fail(ctx, MIOC_EINVAL, "need T1 > T0");
  if (prog->nd > 0 && !d_data) return fail(ctx, MIOC_EINVAL, "the program reads sampled data: d_data missing");
  if (d_Y && !(prog->flags & MIOC_ODE_STATES))
    return fail(ctx, MIOC_EINVAL, "the program was not created with MIOC_ODE_STATES");
  if (d_Jp && !(prog->sens & MIOC_ODE_SENS_P))
    return fail(ctx, MIOC_EINVAL, "the program was not created with MIOC_ODE_SENS_P");
  if (d_Jy0 && !(prog->sens & MIOC_ODE_SENS_Y0))
    return fail(ctx, MIOC_EINVAL, "the program was not created with MIOC_ODE_SENS_Y0");
  if (nu < 0 || nu >= prog->nx) return fail(ctx, MIOC_EINVAL, "need 1 <= nu < the program's nx");
  if (ctx->have_levels && ctx->M != prog->nx - nu)
    return fail(ctx, MIOC_EINVAL, nu ? "the program's nx differs from nu + the levels' number of controls"
                                     : "the program's nx differs from the levels' number of controls");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, MIOC_EHIP, "hipSetDevice failed");
  hipFunction_t fn = nullptr;
  {
    std::lock_guard<std::mutex> lock(prog->mu);
    for (const auto &l : prog->loaded)
      if (l.device == ctx->device) fn = l.fn;
    if (!fn) {
      mioc_ode_program::Loaded l{ctx->device, nullptr, nullptr};
      hipError_t e = hipModuleLoadData(&l.mod, prog->code.data());
      if (e == hipSuccess) {
        e = hipModuleGetFunction(&l.fn, l.mod, kKernelName);
        if (e != hipSuccess) (void)hipModuleUnload(l.mod);
      }
      if (e != hipSuccess) return fail(ctx, MIOC_EHIP, std::string("loading the ODE program: ") + hipGetErrorString(e));
      prog->loaded.push_back(l);
      fn = l.fn;
    }
  }
  const bool euler = prog->integrator == MIOC_ODE_INT_EULER;
  if (euler) {  // forward states [nt][ny][K]
    const int rc = ctx->d_ode_state.grow(ctx, (size_t)K * (size_t)nt * (size_t)prog->ny * sizeof(double), "ODE states");
    if (rc) return rc;
  } else if (d_df || d_Jp || d_Jy0) {  // the state of every substep (Heun / RK4: at its start, implicit: its stage state)
    // [nt * substeps][ny][K], for the backward sweep; a value-only call stores nothing
    // K * nt < 2^62 and per <= 64 * 8 * 8: the product is taken only once it is known to stay below 2^46
    const uint64_t cells = (uint64_t)K * (uint64_t)nt, per = (uint64_t)(prog->substeps * prog->ny) * sizeof(double);
    if (cells > ((uint64_t)1 << 46) / per) return fail(ctx, MIOC_ENOMEM, "the ODE states of all substeps exceed 64 TiB");
    const int rc = ctx->d_ode_state.grow(ctx, (size_t)(cells * per), "ODE states");
    if (rc) return rc;
  }
  int Ki = (int)K, nti = (int)nt, ms = prog->substeps;
  double t0 = T0, tau = (T1 - T0) / (double)nt;  // ODEObjective.jl: tau = (T1 - T0) / nt
  double h = tau / (double)ms;                   // the substep of every scheme but Euler
  double par[kMaxNY + kMaxNP] = {};              // the skeleton's Par: y0[NY], then p[max(NP, 1)]
  if (!prog->scen) {
    for (int r = 0; r < prog->ny; ++r) par[r] = state0[r];
    for (int q = 0; q < prog->np; ++q) par[prog->ny + q] = params[q];
  }
  const double *X = d_x;
  double *ST = ctx->d_ode_state.get();
  const int32_t *gate = ctx->gate;
  // the data pointer and the state output follow the gate, each only in a kernel compiled with it
  // a scenario program takes S and the two device arrays where the others take Par
  int Si = (int)S;
  void *args_euler[14] = {&Ki, &nti, &t0, &tau};
  void *args_rk[18] = {&Ki, &nti, &ms, &t0, &tau, &h};
  void **args = euler ? args_euler : args_rk;
  int na = euler ? 4 : 6;
  if (prog->scen) {
    args[na++] = &Si, args[na++] = &state0, args[na++] = &params;
  } else {
    args[na++] = par;
  }
  args[na++] = &X, args[na++] = &d_J, args[na++] = &d_df, args[na++] = &ST, args[na++] = &gate;
  if (prog->nd > 0) args[na++] = &d_data;
  if (prog->flags & MIOC_ODE_STATES) args[na++] = &d_Y;
  if (prog->sens) args[na++] = &d_Jp, args[na++] = &d_Jy0;  // never an Euler program
  const hipError_t e = hipModuleLaunchKernel(fn, (unsigned)((K + 63) / 64), 1, 1, 64, 1, 1, 0, ctx->stream, args, nullptr);
  if (e != hipSuccess) return fail(ctx, MIOC_EHIP, std::string("launching the ODE program: ") + hipGetErrorString(e));
  return MIOC_OK;
}

int32_t mioc_ode_program_eval_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t K, const double *d_x, int64_t nt,
                                     double T0, double T1, const double *state0, const double *params, double *d_J,
                                     double *d_df) {
  if (ctx && prog && prog->nd > 0)
    return fail(ctx, MIOC_EINVAL, "the program reads sampled data: use mioc_ode_program_eval_bolza_device");
  return program_eval(ctx, prog, 0, K, d_x, nt, T0, T1, 0, state0, params, nullptr, d_J, d_df, nullptr);
}

int32_t mioc_ode_program_eval_mixed_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K,
                                           const double *d_x, int64_t nt, double T0, double T1, const double *state0,
                                           const double *params, double *d_J, double *d_df) {
  if (ctx && nu < 1) return fail(ctx, MIOC_EINVAL, "need 1 <= nu < the program's nx");
  if (ctx && prog && prog->nd > 0)
    return fail(ctx, MIOC_EINVAL, "the program reads sampled data: use mioc_ode_program_eval_bolza_device");
  return program_eval(ctx, prog, nu, K, d_x, nt, T0, T1, 0, state0, params, nullptr, d_J, d_df, nullptr);
}

int32_t mioc_ode_program_eval_bolza_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K,
                                           const double *d_x, int64_t nt, double T0, double T1, const double *state0,
                                           const double *params, const double *d_data, double *d_J, double *d_df,
                                           double *d_Y) {
  return program_eval(ctx, prog, nu, K, d_x, nt, T0, T1, 0, state0, params, d_data, d_J, d_df, d_Y);
}

int32_t mioc_ode_program_eval_scen_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K,
                                          const double *d_x, int64_t nt, double T0, double T1, int64_t S,
                                          const double *d_state0, const double *d_params, const double *d_data,
                                          double *d_J, double *d_df, double *d_Y) {
  if (ctx && S < 1) return fail(ctx, MIOC_EINVAL, "need S >= 1 scenarios and K a multiple of S");
  return program_eval(ctx, prog, nu, K, d_x, nt, T0, T1, S, d_state0, d_params, d_data, d_J, d_df, d_Y);
}

int32_t mioc_ode_program_eval_sens_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K,
                                          const double *d_x, int64_t nt, double T0, double T1, int64_t S,
                                          const double *state0, const double *params, const double *d_data,
                                          double *d_J, double *d_df, double *d_Y, double *d_Jp, double *d_Jy0) {
  return program_eval(ctx, prog, nu, K, d_x, nt, T0, T1, S, state0, params, d_data, d_J, d_df, d_Y, d_Jp, d_Jy0);
}

}  // extern "C"
