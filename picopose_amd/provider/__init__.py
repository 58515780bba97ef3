"""Mirror of the reference's provider/: training-pair assembly on the device (training_batch) and a test image's detection
batch from its RLE records (test_batch)."""
