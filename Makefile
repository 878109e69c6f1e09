# Top-level build: the product library (gfx950 HIP), the same engine with the
# test hooks of include/gvstore_test.h, and the CPU oracle (tests only).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
# bitwise & and | on bools are deliberate in the kernels: no short-circuit
# branches that skip code by the data (DESIGN.md §3 rule 6)
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function -Wno-bitwise-instead-of-logical

LIB := grapevine_amd/libgvstore.so
TESTLIB := grapevine_amd/libgvstore_test.so
SRCS := grapevine_amd/csrc/gvs_engine.hip
HDRS := $(wildcard grapevine_amd/csrc/*.h) include/gvstore.h include/gvstore_test.h

SRHOST := tests/libsrhost.so
EDHOST := tests/libedhost.so
CHACHAHOST := tests/libchachahost.so
AEADHOST := tests/libaeadhost.so
AEADLONGHOST := tests/libaeadlonghost.so
XHOST := tests/libxhost.so
NHOST := tests/libnhost.so
NLONGHOST := tests/libnlonghost.so
CPHOST := tests/libchachapolyhost.so
CPLONGHOST := tests/libchachapolylonghost.so
NINITHOST := tests/libninithost.so

all: $(LIB) $(TESTLIB) $(SRHOST) $(EDHOST) $(CHACHAHOST) $(AEADHOST) $(AEADLONGHOST) $(XHOST) $(NHOST) $(NLONGHOST) $(CPHOST) $(CPLONGHOST) $(NINITHOST) oracle

$(LIB): $(SRCS) $(HDRS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(SRCS) -lrccl

$(TESTLIB): $(SRCS) $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DGVS_TEST_HOOKS -shared -o $@ $(SRCS) -lrccl

# the device signature-check arithmetic built for the CPU (tests/test_sr_host.py)
$(SRHOST): tests/sr_host.cpp grapevine_amd/csrc/gvs_sr25519.h grapevine_amd/csrc/gvs_device.h
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/sr_host.cpp

# the device Ed25519 check (SHA-512, decode, the whole verification) built for
# the CPU (tests/test_ed_host.py)
$(EDHOST): tests/ed_host.cpp grapevine_amd/csrc/gvs_ed25519.h grapevine_amd/csrc/gvs_sr25519.h grapevine_amd/csrc/gvs_device.h
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/ed_host.cpp

# the device challenge stream (ChaCha20 block, draw selection) built for the
# CPU (tests/test_chacha_host.py)
$(CHACHAHOST): tests/chacha_host.cpp grapevine_amd/csrc/gvs_chacha.h grapevine_amd/csrc/gvs_chacha_rounds.h
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/chacha_host.cpp

# the device channel cipher's primitives (AES-256, GF(2^128), the serial
# AES-256-GCM) built for the CPU (tests/test_aead.py)
$(AEADHOST): tests/aead_host.cpp grapevine_amd/csrc/gvs_aead.h grapevine_amd/csrc/gvs_seal_dev.h grapevine_amd/csrc/gvs_crypto.h grapevine_amd/csrc/gvs_device.h
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/aead_host.cpp

# the long channel cipher's schedule (256 thread states stepped through the
# phases of k_aead_long) built for the CPU (tests/test_aead_long.py)
$(AEADLONGHOST): tests/aead_long_host.cpp tests/aead_host.cpp grapevine_amd/csrc/gvs_aead_long.h grapevine_amd/csrc/gvs_aead.h grapevine_amd/csrc/gvs_seal_dev.h grapevine_amd/csrc/gvs_crypto.h grapevine_amd/csrc/gvs_device.h
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/aead_long_host.cpp

# the device X25519 quad ladder (four lane states stepped in a loop) and the
# Noise HKDF built for the CPU (tests/test_x25519.py)
$(XHOST): tests/x25519_host.cpp grapevine_amd/csrc/gvs_x25519.h grapevine_amd/csrc/gvs_ed25519.h grapevine_amd/csrc/gvs_sr25519.h grapevine_amd/csrc/gvs_device.h
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/x25519_host.cpp

# the device Noise IX responder (the three phases of k_noise_ix over four lane
# states, chained with the host ladder and the serial AES-256-GCM) built for
# the CPU (tests/test_noise.py)
$(NHOST): tests/noise_host.cpp tests/aead_host.cpp $(wildcard grapevine_amd/csrc/*.h)
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/noise_host.cpp

# the long responder (phases A and B as above, then k_noise_ix_tail's schedule
# in a loop over the handshakes) built for the CPU (tests/test_noise_long.py)
$(NLONGHOST): tests/noise_long_host.cpp tests/noise_host.cpp tests/aead_host.cpp $(wildcard grapevine_amd/csrc/*.h)
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/noise_long_host.cpp

# the second channel cipher's primitives (the RFC 8439 block function,
# Poly1305 over 26-bit limbs, the serial ChaCha20-Poly1305) built for the CPU
# (tests/test_chachapoly.py)
$(CPHOST): tests/chachapoly_host.cpp grapevine_amd/csrc/gvs_chachapoly.h grapevine_amd/csrc/gvs_chacha_rounds.h grapevine_amd/csrc/gvs_aead.h grapevine_amd/csrc/gvs_seal_dev.h grapevine_amd/csrc/gvs_crypto.h grapevine_amd/csrc/gvs_device.h
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/chachapoly_host.cpp

# the long ChaCha20-Poly1305 schedule (256 thread states stepped through the
# phases of k_chachapoly_long) built for the CPU (tests/test_chachapoly_long.py)
$(CPLONGHOST): tests/chachapoly_long_host.cpp grapevine_amd/csrc/gvs_chachapoly_long.h grapevine_amd/csrc/gvs_chachapoly.h grapevine_amd/csrc/gvs_chacha_rounds.h grapevine_amd/csrc/gvs_aead_long.h grapevine_amd/csrc/gvs_aead.h grapevine_amd/csrc/gvs_seal_dev.h grapevine_amd/csrc/gvs_crypto.h grapevine_amd/csrc/gvs_device.h
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/chachapoly_long_host.cpp

# the device Noise IX initiator (the four phases of k_noise_ixi over four lane
# states, chained with the host ladder and the serial ciphers) built for the
# CPU (tests/test_noise_init.py)
$(NINITHOST): tests/noise_init_host.cpp tests/noise_host.cpp tests/aead_host.cpp $(wildcard grapevine_amd/csrc/*.h)
	$(HIPCC) -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -o $@ tests/noise_init_host.cpp

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(LIB) $(TESTLIB) $(SRHOST) $(EDHOST) $(CHACHAHOST) $(AEADHOST) $(AEADLONGHOST) $(XHOST) $(NHOST) $(NLONGHOST) $(CPHOST) $(CPLONGHOST) $(NINITHOST)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
