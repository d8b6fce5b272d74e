// goldilocks_verifier.hpp — the verifier of the 64-bit field's claim in the C++ host (cli/src/main.rs:168-178 `claim.verify`): the mirror of
// goldilocks._verify, check for check, in its order and in its words.  Free of the device runtime.
#pragma once
#include <cstdint>
#include <vector>

#include "air_plain.hpp"
#include "goldilocks_prover.hpp"

namespace ssh {
namespace gl {

// The proof blob of ssh_gl_prove* (host_capi.cpp) -> Proof.  The blob is untrusted: every count is checked against the words left before
// anything is read, and what is refused is refused by name ("proof blob: ...").
Proof parse_proof_blob(const uint64_t *blob, uint64_t len);

// -> the query positions, or a std::runtime_error naming the failed check (goldilocks.VerificationError's text)
std::vector<uint64_t> verify(const PlainAir &air, const Options &opt, uint32_t hash_option, const Digest &seed, const Proof &proof, uint32_t required_security_bits);

}  // namespace gl
}  // namespace ssh
