# Test programs that need the reference project's tree (REFERENCE), which is
# not part of this repository: the reference-side adapter (integration/)
# compiled against the reference's own headers, and the reference's own PDF /
# JBIG2 unit tests compiled where they lie against integration/pdf_hip.c and
# jbig2_hip.c instead of MuPDF / jbig2dec.  They are built into oracle/_ref/
# (kept out of git) wherever the reference tree is present, and run from
# there by tests/test_c_abi_gpu.py and tests/test_pdf.py; a machine without
# the tree runs the programs built elsewhere and carried over in oracle/_ref/.
# Included by the top-level Makefile (CC, PKG, LIB, ORACLE_LIB and REFERENCE
# come from it).

REFDIR    := oracle/_ref
ADAPTER    := $(REFDIR)/adapter_ops
REF_PDF_TESTS := $(REFDIR)/ref_pdf_reader_test $(REFDIR)/ref_pdf_writer_test \
                 $(REFDIR)/ref_jbig2_decode_test
# from oracle/_ref/ to the product library and the oracle
REF_RPATH  := -Wl,-rpath,'$$ORIGIN/../../$(PKG)/lib'
REF_RPATH_ORACLE := -Wl,-rpath,'$$ORIGIN/../_build'

.PHONY: adapter
adapter: $(ADAPTER) $(REF_PDF_TESTS)

$(ADAPTER): tests/c/adapter_main.c tests/c/pages.h integration/backend_hip.c integration/backend_hip.h \
            integration/hip_frame.h include/unpaper_hip.h oracle/oracle.h $(LIB) $(ORACLE_LIB)
	@test -f $(REFERENCE)/imageprocess/image.h || { echo "adapter: no reference headers under $(REFERENCE)"; exit 1; }
	@mkdir -p $(REFDIR)
	$(CC) -O2 -std=gnu11 -Wall -Wno-unused-variable -I$(REFERENCE) -Iinclude -Iintegration \
	  tests/c/adapter_main.c integration/backend_hip.c -o $@ \
	  -L$(PKG)/lib -L oracle/_build -lunpaper_hip -loracle -lm $(REF_RPATH) $(REF_RPATH_ORACLE)

$(REFDIR)/ref_pdf_%_test: integration/pdf_hip.c include/unpaper_hip.h $(LIB)
	@test -f $(REFERENCE)/tests/pdf_$*_test.c || { echo "ref pdf tests: no reference tree under $(REFERENCE)"; exit 1; }
	@mkdir -p $(REFDIR)
	$(CC) -O2 -std=gnu11 -Wall -Wno-unused-variable -Wno-unused-function -I$(REFERENCE) -Iinclude \
	  $(REFERENCE)/tests/pdf_$*_test.c integration/pdf_hip.c -o $@ \
	  -L$(PKG)/lib -lunpaper_hip -lm $(REF_RPATH)

$(REFDIR)/ref_jbig2_decode_test: integration/jbig2_hip.c integration/pdf_hip.c include/unpaper_hip.h $(LIB)
	@test -f $(REFERENCE)/tests/jbig2_decode_test.c || { echo "ref jbig2 test: no reference tree under $(REFERENCE)"; exit 1; }
	@mkdir -p $(REFDIR)
	$(CC) -O2 -std=gnu11 -Wall -Wno-unused-variable -Wno-unused-function -DUNPAPER_WITH_JBIG2 -DUNPAPER_WITH_PDF \
	  -I$(REFERENCE) -Iinclude $(REFERENCE)/tests/jbig2_decode_test.c integration/jbig2_hip.c integration/pdf_hip.c \
	  -o $@ -L$(PKG)/lib -lunpaper_hip -lm $(REF_RPATH)
