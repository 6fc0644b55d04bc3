// Host arithmetic and planning of the engine (hbbft_amd/csrc/host_fr.hpp, wire_host.hpp,
// ack_plan.hpp) as a stand-alone program: one command per line on stdin, one line of tokens per
// command on stdout (numbers in hex).  tests/test_engine_host.py builds it with the address and
// undefined-behaviour sanitizers and compares its output with the Python oracle.
//   lagrange ncomb m x...      -> status per combine; lambdas; host_gls_digits of them;
//                                 host_interp_digits g2 (status, digits); the same for g1
//   digits n scalar...         -> per scalar: 4 base-|x| digits, then rem and quotient of / x^2 (2 + 2 words)
//   parse nfe hexbytes         -> flag, then 12 * nfe words
//   order n y...               -> the permutation
//   dedup nack nparts (part x)... -> ok; nrow; row_part; row_x; row_of
//   planfd n t (slot y)...     -> nfd; slot; y0; off; len; npts; epos (n); |fd_acks|; fd_acks; |other|; other
//   plandrain n t use_fd (slot y)... -> plan_drain's plan as planfd prints it, |epos| before epos; |order|; order
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ack_plan.hpp"
#include "host_fr.hpp"
#include "wire_host.hpp"

namespace {
void put(uint64_t v) { std::printf("%llx ", (unsigned long long)v); }
void put4(const uint64_t* w) { std::printf("%016llx%016llx%016llx%016llx ", (unsigned long long)w[3], (unsigned long long)w[2], (unsigned long long)w[1], (unsigned long long)w[0]); }
void put_vec(const std::vector<uint32_t>& v) {
  for (uint32_t x : v) put(x);
}
void put_plan(const FdPlan& P, bool epos_len) {
  put(P.slot.size());
  put_vec(P.slot);
  put_vec(P.y0);
  put_vec(P.off);
  put_vec(P.len);
  put(P.npts);
  if (epos_len) put(P.epos.size());
  put_vec(P.epos);
  put(P.fd_acks.size());
  put_vec(P.fd_acks);
  put(P.other.size());
  put_vec(P.other);
}
bool get4(std::istream& in, uint64_t* w) {  // a scalar of up to 64 hex digits
  std::string h;
  if (!(in >> h) || h.size() > 64) return false;
  h = std::string(64 - h.size(), '0') + h;
  for (int i = 0; i < 4; i++) w[3 - i] = std::stoull(h.substr(16 * i, 16), nullptr, 16);
  return true;
}
}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    in >> std::hex;
    if (cmd == "lagrange") {
      size_t ncomb = 0, m = 0;
      in >> ncomb >> m;
      std::vector<uint32_t> xs(ncomb * m);
      for (auto& x : xs) in >> x;
      if (!in) return 2;
      std::vector<uint64_t> lam(ncomb * m * 4), dg(ncomb * m * 4);
      std::vector<int> st(ncomb);
      host_lagrange(xs.data(), ncomb, m, lam.data(), st.data());
      for (int s : st) put((uint64_t)s);
      for (size_t k = 0; k < ncomb * m; k++) put4(&lam[k * 4]);
      host_gls_digits(lam.data(), ncomb * m, dg.data());
      for (uint64_t d : dg) put(d);
      for (int g1 = 0; g1 < 2; g1++) {
        std::vector<int> st2(ncomb, -1);
        host_interp_digits(xs.data(), ncomb, m, dg.data(), st2.data(), g1 != 0);
        for (int s : st2) put((uint64_t)s);
        for (uint64_t d : dg) put(d);
      }
    } else if (cmd == "digits") {
      size_t n = 0;
      in >> n;
      for (size_t k = 0; k < n; k++) {
        uint64_t q[4], dg[4], rem[2];
        if (!get4(in, q)) return 2;
        host_gls_digits(q, 1, dg);
        for (uint64_t d : dg) put(d);
        host_div_x2(q, rem);
        put(rem[0]), put(rem[1]), put(q[0]), put(q[1]);
        put(q[2] | q[3]);  // the quotient fits two words
      }
    } else if (cmd == "parse") {
      int nfe = 0;
      std::string h;
      in >> nfe >> h;
      if (!in || (nfe != 1 && nfe != 2) || h.size() != (size_t)96 * nfe) return 2;
      std::vector<uint8_t> b(48 * nfe);
      for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
      std::vector<uint32_t> w(12 * nfe);
      uint8_t f = 0xff;
      parse_compressed(b.data(), nfe, w.data(), f);
      put(f);
      put_vec(w);
    } else if (cmd == "order") {
      size_t n = 0;
      in >> n;
      std::vector<uint32_t> ys(n), order;
      for (auto& y : ys) in >> y;
      if (!in) return 2;
      order_by_y(n, ys.data(), order);
      put_vec(order);
    } else if (cmd == "dedup") {
      size_t nack = 0, nparts = 0;
      in >> nack >> nparts;
      std::vector<uint32_t> part(nack), xs(nack), rp, rx, ro;
      for (size_t a = 0; a < nack; a++) in >> part[a] >> xs[a];
      if (!in) return 2;
      const bool ok = dedup_rows(nack, nparts, part.data(), xs.data(), rp, rx, ro);
      put(ok);
      if (ok) {
        put(rp.size());
        put_vec(rp);
        put_vec(rx);
        put_vec(ro);
      }
    } else if (cmd == "planfd") {
      size_t n = 0;
      int t = 0;
      in >> n >> t;
      std::vector<uint32_t> slot(n), ys(n);
      for (size_t a = 0; a < n; a++) in >> slot[a] >> ys[a];
      if (!in) return 2;
      FdPlan P;
      plan_fd(n, slot, ys.data(), t, P);
      put_plan(P, false);
    } else if (cmd == "plandrain") {
      size_t n = 0;
      int t = 0, use_fd = 0;
      in >> n >> t >> use_fd;
      std::vector<uint32_t> slot(n), ys(n);
      for (size_t a = 0; a < n; a++) in >> slot[a] >> ys[a];
      if (!in) return 2;
      FdPlan P;  // a used plan and order going in: plan_drain starts from nothing
      std::vector<uint32_t> order(3, 0xdeadbeefu);
      plan_fd(n, slot, ys.data(), t, P);
      plan_drain(n, slot, ys.data(), t, use_fd != 0, P, order);
      put_plan(P, true);
      put(order.size());
      put_vec(order);
    } else {
      return 2;
    }
    std::printf("\n");
  }
  return 0;
}
